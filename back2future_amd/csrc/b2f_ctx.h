// Internal to libb2f.so: the context behind the opaque b2f_ctx of include/b2f.h, shared by the C-ABI layer
// (b2f_api.hip), the kernel test entries (b2f_ops.hip) and the host-buffer pipeline (b2f_pipeline.hip).
#pragma once
#include "../../include/b2f.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "b2f_host.h"
#include "b2f_internal.h"

namespace b2f {

// error reporting of the C ABI: message kept per thread for b2f_last_error(), returns 1
int api_fail(const std::string &m);
const std::string &api_error();


// The kernels that can run a conv layer; each reads its own packing of the layer's weights (b2f_api.hip: kKernels has one row per kernel).
enum ConvKernel {
    K_DIRECT = 0,   // direct implicit GEMM on the fp32 MFMA, stride 1 / 2 (b2f_conv.hip)
    K_NARROW2,      // VALU kernel for 2 outputs (b2f_glue.hip)
    K_WINO2,        // Winograd F(2x2,3x3) (b2f_wino.hip)
    K_C16,          // 16 -> 16 stride-1 kernel (b2f_conv16.hip)
    K_C16S2,        // 16 -> 32 stride-2 kernel (b2f_conv16.hip)
    K_WINO4,        // Winograd F(4x4,3x3) (b2f_wino4.hip)
    K_BF6,          // direct implicit GEMM on the bf16 pipe with split fp32 operands (b2f_convb.hip)
    K_S2B,          // stride-2 loader / consumer kernel on the bf16 pipe (b2f_s2b.hip)
    K_W1B,          // 1-D Winograd F(4,3) loader / consumer kernel on the bf16 pipe (b2f_w1b.hip)
    K_WINO6,        // Winograd F(6x6,3x3) (b2f_wino6.hip)
#if B2F_EXPERIMENTS
    K_WINO4S,       // split weights the F(4x4) launcher reads with wino4_split / wino4_hybrid (b2f_wino4s.hip)
    K_WINO2S,       // split weights it reads with wino2_split (b2f_wino2s.hip)
#endif
    K_COUNT
};

struct PackedConv {
    int nseg = 1;
    int chunks[2] = {0, 0};
    int cout = 0;
    ConvKernel base = K_DIRECT;    // the layer's kernel while no option and no map size sends a launch elsewhere (choose_kernel)
    // One packing per kernel that may run the layer, offsets in floats into the weight buffer; nblk = 0: the layer has none.  Next to the base
    // packing: F(4x4) layers carry an F(2x2) one for small maps (one 16 x 32-pixel block per CU does not fill the chip below ~64 x 64 pixels;
    // measured at 32 x 60: 0.05 ms vs 0.14 ms), and the optional ones exist only while an option reads them.
    struct Packing {
        size_t w_off = 0, b_off = 0;
        int nt = 0, nblk = 0;      // 32-wide N tiles per block, N blocks: the bias is nblk * nt * 32 floats
    } pk[K_COUNT];
    bool has(ConvKernel k) const { return pk[k].nblk != 0; }
    int nchunks() const { return chunks[0] + (nseg > 1 ? chunks[1] : 0); }
};

// The options that decide which kernel runs a conv layer and how it is launched (b2f_set_option; seeded once from the environment in
// b2f_init, never read from it on the hot path): what choose_kernel reads.  b2f_op_conv3x3 passes a copy with its overrides.
struct KernelOpts {
    int wino8 = 1;                 // F(2x2) one-N-tile launches of at most one block per CU run the eight-wave form (conv3x3_wino8; same bits)
    int wino_split_pixels = 512;   // F(2x2) launches on maps of at most this many pixels run one block per 32-output N tile (same bits;
                                   // level 7 of a full-HD triplet: 64 tiles per launch at batch 16 -- 0.25 -> 0.20 ms for its six layers)
    int wino4_min_pixels = 4096;   // F(4x4) for maps of at least this many pixels, F(2x2) below: depends on the map size
                                   // only, so a triplet's result does not depend on the batch it is computed in
    int adaptive_kernels = -1;     // -1 (default): per launch for single-triplet calls, by map size for batches; 0: by map size always;
                                   // 1: choose the Winograd variant per launch by block rounds on the 256 CUs (faster for
                                   // single triplets / small batches; results then depend on the batch size at 1e-6 level)
    int bf16_direct = 2;           // the 16-channel layers of the head on the bf16 matrix pipe with exactly split fp32 operands: 0 = fp32-MFMA kernels,
                                   // 1 = the 16 -> 16 layer alone (b2f_conv16b.hip), 2 = 16 -> 16 + 16 -> 32 stride 2 fused, the map between them in LDS (b2f_head.hip)
    int bf16_conv_min_pixels = 65536;   // bf16_conv = 2: 32-output stride-1 layers on maps of at least this many pixels leave the F(4x4) kernel
    int bf16_conv = 1;             // 1 (default): the direct (stride-2) layers on the bf16 matrix pipe with split fp32 operands (b2f_convb.hip);
                                   // 2: also the 32-output stride-1 layers of large maps, 3: every F(4x4)-class layer of large maps (experiments: measured
                                   // slower than the F(4x4) kernel, profiles/r04_bf16_direct_notes.txt (4)); 0: fp32-MFMA kernel
    int wino2_split = 0;           // F(4x4)-class layers, blocks of 64 outputs: 1 = Winograd F(2x2) on the bf16 matrix pipe with exactly split
                                   // fp32 operands (b2f_wino2s.hip) on maps of at least wino4_min_pixels pixels
    int wino4_hybrid = 0;          // F(4x4) two-N-tile blocks: this many of a wave's nine xi steps on the bf16 pipe with split operands (needs the
                                   // split packing: setting it > 0 packs it); 0 = all on the fp32 MFMA
    int wino4_split = 0;           // F(4x4) layers with two full N tiles per block: 1 = on the bf16 matrix pipe with exactly split fp32 operands
                                   // (b2f_wino4s.hip; fp32-level accuracy, measured no faster: profiles/r04_wino4s_notes.txt), 0 = on the fp32 MFMA
    int wino6 = 1;                 // F(4x4)-class layers on maps of at least wino6_min_pixels pixels: 1 = Winograd F(6x6,3x3) on the fp32 MFMA (csrc/b2f_wino6.hip):
                                   // blocks of 64 outputs, a last block of 32 when the outputs are <= 32 mod 64
    int wino6_min_pixels = 16384;  // ... below that the F(4x4) kernel (items of 12 x 48 pixels quantise small maps badly)
    int wino1d = 0;                // F(4x4)-class layers (stride 1, more than 32 outputs, maps of at least wino4_min_pixels pixels): 1 = one-dimensional
                                   // Winograd F(4,3) on the bf16 matrix pipe with exactly split fp32 operands, loader / consumer persistent blocks
                                   // (b2f_w1b.hip); 0 = the fp32-MFMA F(4x4) kernel of rounds 1-4 (b2f_wino4.hip)
    int s2_tile_groups = 1;        // ... launches that cannot fill the chip: one output tile per block (conv3x3_s2b<1, 1>, ConvLaunch::nsplit); same bits
    int s2_loader = 1;             // stride-2 layers on the bf16 pipe (bf16_conv >= 1): 1 = those of at least 64 input channels on the loader / consumer kernel
                                   // that computes all outputs of a tile (b2f_s2b.hip), 2 = all of them, 0 = conv3x3_bf6 (b2f_convb.hip)
    int wino4_persistent = 1;      // F(4x4) kernel: 1 = persistent blocks (one per CU, K pipeline continues across tiles), 0 = one tile per block, > 1 = that many persistent blocks (tests)
    int s2_tiles_per_block = 0;    // direct stride-2 kernel: tiles chained per block (0 = launcher's rule; bit-identical either way)
};

struct ProfEvent {
    int name;
    hipEvent_t a, b;
};

struct GraphKey {
    const void *in;
    float *flow, *occ, *est3;
    int kind, B, H, W;
    int rule;                      // kernel-choice rule the captured launches follow (1 = per launch: a single-triplet request), part of the key
    int seq;                       // 1 = sequence mode (in = B + 2 frames): never the graph of a triplet call with the same pointers and B
    const void *ring = nullptr;    // stream mode (StreamPass): the stream's device block; in = the frame slot of the pushed frames ...
    int phase = 0;                 // ... 1 + 2 * ring slot + ready: a stream captures one graph per ring phase, and one without the decoders
    float *past = nullptr;         // the past-flow output: a graph with the past decoder chain is never the graph of a call without it
    bool operator<(const GraphKey &o) const
    {
        return std::tie(in, flow, occ, est3, kind, B, H, W, rule, seq, ring, phase, past) <
               std::tie(o.in, o.flow, o.occ, o.est3, o.kind, o.B, o.H, o.W, o.rule, o.seq, o.ring, o.phase, o.past);
    }
};

// One push of a stream (b2f_stream) as the forward pass sees it: the pyramid of the B = cams pushed frames (dev_in of forward_device: their
// frame slot) goes into pyr[3..7], the ring slot of this push; with `ready` the pass goes on from the cost volume, reading the three
// frames of every camera's triplet from the ring slots of pushes k - 2, k - 1 and k (past / ref / fut: per level, B images each) and, for
// the Hard models' est[3], the frames of push k - 2 as the pyramid read them (frame_past, frame_kind).
struct StreamPass {
    const void *ring = nullptr;
    int slot = 0;
    bool ready = false;
    float *pyr[8] = {nullptr};
    const float *past[8] = {nullptr}, *ref[8] = {nullptr}, *fut[8] = {nullptr};
    const void *frame_past = nullptr;
    int frame_kind = B2F_IN_UNIT;
    // a stream opened with B2F_STREAM_WARP: the caller's own frames (H0 x W0, raw_kind bytes or floats, B images 3 planes apart) of
    // pushes k - 2, k - 1 and k, which the warp of a push samples as im1 / im2 / im3; nullptr on a stream without the flag
    const void *raw_past = nullptr, *raw_ref = nullptr, *raw_fut = nullptr;
    int raw_kind = B2F_IN_UNIT;
};

// One of the two buffer sets the host-buffer entry point (b2f_compute_flow_batch) alternates between: while the
// kernels of sub-batch k run on set k & 1, the uploads of k + 1 and the downloads of k - 1 use the other one.
struct HostSlot {
    char *dev = nullptr;        // device blob, carved below
    size_t dev_bytes = 0;
    char *pin = nullptr;        // pinned staging blob
    size_t pin_bytes = 0;
    unsigned char *d_u8 = nullptr;   // 8-bit transport of the input planes (see pack_u8_piece)
    float *d_up = nullptr, *d_tmp = nullptr, *d_in = nullptr, *d_flow = nullptr, *d_est3 = nullptr;
    float *d_flow32 = nullptr;       // flow at H0 x W0 (fp32; f64 path: before the sc_w / sc_h factors); = d_flow without a rescale
    float *d_occ = nullptr;          // f32 path of a Hard model with occ_prob: skip_occs[3] at the network size (Soft: it is d_est3)
    float *d_prob = nullptr;         // f32 path: occ_prob at H0 x W0; unused without a rescale (the network's planes go down as they are)
    unsigned char *d_fo = nullptr, *d_bo = nullptr;
    unsigned char *d_rgb = nullptr;  // rgb requests: the pictures of the sub-batch (3 bytes per pixel) ...
    double *d_max = nullptr;         // ... and the maximum every one of them was scaled with
    unsigned char *h_u8 = nullptr;
    float *h_in = nullptr, *h_flow32 = nullptr, *h_prob = nullptr;
    unsigned char *h_fo = nullptr, *h_bo = nullptr, *h_rgb = nullptr;
    double *h_max = nullptr;
    // score requests: the ground truth of the sub-batch (uploaded with the frames) and its records; staging for pageable buffers
    float *d_gt = nullptr, *h_gt = nullptr;
    unsigned char *d_valid = nullptr, *d_gtocc = nullptr, *h_valid = nullptr, *h_gtocc = nullptr;
    unsigned long long *d_score = nullptr, *h_score = nullptr;
    // warp requests: the warped neighbours of the sub-batch (in the request's element type) and its photometric records
    void *d_warp = nullptr, *h_warp = nullptr;
    unsigned long long *d_photo = nullptr, *h_photo = nullptr;
    // past-flow requests: skip_ubfs[3] at the network size, at H0 x W0 (= d_past without a rescale) and the staging of a pageable buffer
    float *d_past = nullptr, *d_past32 = nullptr, *h_past = nullptr;
    hipEvent_t ev_in = nullptr, ev_comp = nullptr, ev_out = nullptr;
};

// Where computeFlow's outputs go (host pointers for b2f_compute_flow*, device pointers for b2f_compute_flow*_device).  The
// f64 path (flow64, both masks required) is the b2f_compute_flow* entries'; the f32 path (flow32) writes the same flow
// rounded to fp32 and, when not nullptr, the occlusion probabilities and the masks.  rgb (f32 path only): the flow pictures of
// b2f_compute_flow*_rgb (xy2rgb of the f32 flow, launch_flow_rgb) in rgb_layout with max_norm, rgb_max their maxima; the flow itself
// is then optional.  scores (f32 path only): the records of b2f_compute_flow*_score (launch_flow_score of the f32 flow and occ_prob
// against gt_flow / valid / gt_occ, which are inputs that travel with the outputs they belong to); the flow is optional there too.
// warped / photo (f32 path only): the outputs of b2f_compute_flow*_warp (launch_flow_warp of the f32 flow, occ_prob and the request's
// own frames with flow_scale); at least one is required, everything else is optional.  past32 (f32 path only): the past flow of a Soft
// model, skip_ubfs[3], rescaled like flow32; own_past: the warp of a warp request places the past frame's samples with that past flow
// (on the device whether or not past32 is asked for).  Either one makes the forward pass run the past-flow decoder chain.
struct FlowOutputs {
    double *flow64 = nullptr;
    float *flow32 = nullptr, *occ_prob = nullptr;
    unsigned char *fwd_occ = nullptr, *bwd_occ = nullptr;
    unsigned char *rgb = nullptr;
    double *rgb_max = nullptr;
    double max_norm = 0.0;
    int rgb_layout = B2F_RGB_PLANAR;
    bool pictures = false;         // an rgb request: rgb is required (check_request), flow32 is not
    unsigned long long *scores = nullptr;
    const float *gt_flow = nullptr;
    const unsigned char *valid = nullptr, *gt_occ = nullptr;
    double flow_scale = 0.0;
    bool scoring = false;          // a score request: scores and gt_flow are required, flow32 is not
    void *warped = nullptr;        // n x 2 x 3 x H0 x W0 of warped_kind (B2F_IN_UNIT floats or B2F_IN_U8 bytes)
    int warped_kind = B2F_IN_UNIT;
    unsigned long long *photo = nullptr;
    bool warping = false;          // a warp request: warped or photo is required, flow32 is not
    float *past32 = nullptr;
    bool own_past = false;
    bool want_past() const { return past32 != nullptr || own_past; }
    bool f32() const { return flow64 == nullptr; }
    // the outputs of triplets b, b + 1, ... (planes of hw0 pixels); nullptr stays nullptr
    FlowOutputs from_triplet(size_t b, size_t hw0) const
    {
        auto at = [](auto *p, size_t off) { return p ? p + off : p; };
        return {at(flow64, b * 2 * hw0), at(flow32, b * 2 * hw0), at(occ_prob, b * 2 * hw0), at(fwd_occ, b * hw0), at(bwd_occ, b * hw0),
                at(rgb, b * 3 * hw0), at(rgb_max, b), max_norm, rgb_layout, pictures,
                at(scores, b * B2F_SCORE_WORDS), at(gt_flow, b * 2 * hw0), at(valid, b * hw0), at(gt_occ, b * hw0), flow_scale, scoring,
                warped ? (void *)((char *)warped + b * 6 * hw0 * (warped_kind == B2F_IN_U8 ? 1 : 4)) : nullptr, warped_kind,
                at(photo, b * B2F_PHOTO_WORDS), warping, at(past32, b * 2 * hw0), own_past};
    }
};

// the outputs of a b2f_*compute_flow_*_rgb entry
inline FlowOutputs rgb_outputs(unsigned char *rgb, double *max_used, double max_norm, int layout, float *flow, unsigned char *fwd_occ,
                               unsigned char *bwd_occ)
{
    return {nullptr, flow, nullptr, fwd_occ, bwd_occ, rgb, max_used, max_norm, layout, true};
}

// the outputs (and the ground truth) of a b2f_*compute_flow_*_score entry
inline FlowOutputs score_outputs(double flow_scale, const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                                 unsigned long long *scores, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ)
{
    FlowOutputs o{nullptr, flow, nullptr, fwd_occ, bwd_occ};
    o.scores = scores; o.gt_flow = gt_flow; o.valid = valid; o.gt_occ = gt_occ; o.flow_scale = flow_scale; o.scoring = true;
    return o;
}

// the outputs of a b2f_*compute_flow_*_warp entry; in_kind: the element type of the request's frames, and so of warped
inline FlowOutputs warp_outputs(double flow_scale, int in_kind, void *warped, unsigned long long *photo, float *flow, float *occ_prob,
                                unsigned char *fwd_occ, unsigned char *bwd_occ)
{
    FlowOutputs o{nullptr, flow, occ_prob, fwd_occ, bwd_occ};
    o.flow_scale = flow_scale; o.warped = warped; o.warped_kind = in_kind; o.photo = photo; o.warping = true;
    return o;
}

// the outputs of a b2f_*compute_flow_*_past entry: those of the _f32 entries and the past flow (nullptr: a plain _f32 request)
inline FlowOutputs past_outputs(float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ)
{
    FlowOutputs o{nullptr, flow, occ_prob, fwd_occ, bwd_occ};
    o.past32 = past_flow;
    return o;
}

// the outputs of a b2f_*compute_flow_*_warp_past entry: a warp request whose past frame follows the model's own past flow
inline FlowOutputs warp_past_outputs(double flow_scale, int in_kind, void *warped, unsigned long long *photo, float *flow, float *past_flow,
                                     float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ)
{
    FlowOutputs o = warp_outputs(flow_scale, in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ);
    o.past32 = past_flow; o.own_past = true;
    return o;
}

// One computeFlow call, whichever of the entry points it came through: n triplets (im1..im3, n x 3 x H0 x W0 each) or, with seq, the
// n + 2 frames of a sequence in im1; inputs B2F_IN_UNIT (floats in [0,1]) or B2F_IN_U8 (bytes).  req: the request's triplet count the
// kernel rule follows (0: n; b2f_multi passes the caller's n to its shards).  who names the entry point in messages.
struct FlowRequest {
    int n = 0;
    bool seq = false;
    int in_kind = B2F_IN_UNIT;
    const void *im1 = nullptr, *im2 = nullptr, *im3 = nullptr;
    int H0 = 0, W0 = 0;
    FlowOutputs o;
    int req = 0;
    const char *who = "";
    b2f_stream *stream = nullptr;   // a push: im1 holds the n = cams new frames, the other two frames of every triplet are the stream's
};

// n = cams frames pushed into st.  A stream is a clip: the kernel rule is a batch's (req >= 2) with one camera too, so that push k gives
// the bits of output k - 3 of the sequence entries.
inline FlowRequest push_request(const char *who, b2f_stream *st, int cams, int in_kind, const void *frames, int H0, int W0, const FlowOutputs &o)
{
    return {cams, false, in_kind, frames, nullptr, nullptr, H0, W0, o, std::max(cams, 2), who, st};
}

inline FlowRequest batch_request(const char *who, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                 const FlowOutputs &o)
{
    return {n, false, in_kind, im1, im2, im3, H0, W0, o, 0, who};
}

// T frames hold T - 2 triplets (0 below three frames: check_request refuses the sequence)
inline FlowRequest sequence_request(const char *who, int T, int in_kind, const void *frames, int H0, int W0, const FlowOutputs &o)
{
    return {T >= 3 ? T - 2 : 0, true, in_kind, frames, nullptr, nullptr, H0, W0, o, 0, who};
}

// The word every byte a kernel has no business touching holds in the guarded test set-ups: a quiet NaN whose payload no arithmetic
// produces.  Compared on bits.
constexpr uint32_t kGuardWord = 0x7fc0a5a5u;

// One guard of the arena (option arena_guard): floats [off, off + len) of the arena.  An "after" guard starts at the end of buffer `buffer`
// of the plan (the buffer's own slack included, e.g. the record's + 64) and covers the rounding of its size to 64 floats and the arena_guard
// floats behind that; the one "before" guard is the arena_guard floats in front of buffer 0.
struct ArenaGuard {
    size_t off, len;
    int buffer;
    bool before;
    const char *name;
};

// One buffer of the generic executor's own layout of the arena (b2f_graph.hip, option arena_guard), as Plan::Buf describes a plan's: where
// it ends, where the next one may start at the earliest (end rounded to 64 floats + the guard), and its role and level, e.g. "occ.in[4]".
struct GraphBuf {
    size_t end, next;
    std::string name;
};

// A device buffer of the kernel test entries (b2f_op_*): kGuardFloats floats of kGuardWord on each side of the n floats handed to the
// kernel, which start as kGuardWord too, so that an element the kernel does not write shows.  p is 256-byte aligned.  check(), after the
// stream has been synchronised, fails with the buffer's name, the side and the offset of the first guard word that changed.
struct DevBuf {
    static constexpr size_t kGuardFloats = 4096;
    float *p = nullptr;
    float *raw = nullptr;
    size_t n = 0;
    const char *name = "";
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (raw) (void)hipFree(raw); }
    int alloc(size_t count, const char *what);
    int check() const;
};

// The device buffers of one kernel test entry (b2f_op_*, b2f_ops.hip): every one is a DevBuf the scope owns, and finish() checks every one
// of them, so an entry keeps no list of its buffers and cannot leave one out.  Sizes are in elements of T and are rounded up to whole
// floats, (bytes + 3) / 4: the up-to-3-byte tail of a byte buffer is not watched.  An optional buffer is one the entry never asks for.
class OpStage {
public:
    OpStage(b2f_ctx *c, std::string fn) : c_(c), fn_(std::move(fn)) {}
    // refuses a null context, or !args_ok, with "<fn>: <what>"; then hipSetDevice
    int begin(bool args_ok = true, const char *what = "null argument");
    // *dev: a buffer that holds host[0 .. n); the copy blocks, so it is complete before the entry's first launch
    template <class T> int in(const T *host, size_t n, const char *name, T **dev) { return typed(host, n * sizeof(T), name, dev); }
    // *dev: a buffer of n elements that holds kGuardWord
    template <class T> int out(size_t n, const char *name, T **dev) { return typed(nullptr, n * sizeof(T), name, dev); }
    // hipGetLastError, hipStreamSynchronize of the context's stream, then check() of every buffer in allocation order
    int finish();
    // dev[0 .. n) to the host; refused before finish()
    template <class T> int get(T *host, const T *dev, size_t n) const { return download(host, dev, n * sizeof(T)); }

private:
    int stage(const void *host, size_t bytes, const char *name, void **dev);
    template <class T> int typed(const void *host, size_t bytes, const char *name, T **dev)
    {
        void *p = nullptr;
        const int rc = stage(host, bytes, name, &p);
        *dev = static_cast<T *>(p);
        return rc;
    }
    int download(void *host, const void *dev, size_t bytes) const;
    b2f_ctx *c_;
    std::string fn_;
    std::deque<DevBuf> bufs_;   // never moves an element: DevBuf stays non-copyable
    bool finished_ = false;
};
// the sizes an op entry accepts: three positive factors whose product is at most 2^26 elements
inline bool small_dims(long long a, long long b, long long c) { return a >= 1 && b >= 1 && c >= 1 && a * b * c <= (1LL << 26); }

// Context-owned device workspace of the device entries (b2f_compute_flow_device / _sequence_device): grows, never shrinks.
struct DevWork {
    char *dev = nullptr;
    size_t bytes = 0;
};

// Host work items of the pipeline, cut into pieces and spread over a pool of threads.
enum { JOB_COPY = 0, JOB_F32_TO_F64 = 1, JOB_PACK_U8 = 2 };
struct CopyJob {
    void *dst;
    const void *src;
    size_t bytes;                     // of the source
    int kind = JOB_COPY;
    double scale = 1.0;               // JOB_F32_TO_F64: dst = (double)src * scale   (back2future.lua:83-84)
    std::atomic<int> *inexact = nullptr;   // JOB_PACK_U8: set when a value is not k / 255
};

// 8-bit transport: image.load hands computeFlow floats that came from 8-bit files, i.e. k / 255.  Such a plane
// crosses the link as bytes (a quarter of the traffic of a path that is PCIe-bound) and is rebuilt on the device
// by the same correctly rounded division, but only if that reproduces every float of it bit for bit; one other
// value (or -0, NaN, ...) and the triplet is uploaded as floats instead.
inline bool pack_u8_piece(unsigned char *d, const float *s, size_t n)
{
    uint32_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const float v = s[i];
        int k = (int)(v * 255.0f + 0.5f);
        k = k < 0 ? 0 : (k > 255 ? 255 : k);
        const float r = (float)k / 255.0f;
        uint32_t vb, rb;
        memcpy(&vb, &v, 4);
        memcpy(&rb, &r, 4);
        bad |= vb ^ rb;
        d[i] = (unsigned char)k;
    }
    return bad == 0;
}

inline void run_piece(const CopyJob &j)
{
    if (j.kind == JOB_COPY) {
        memcpy(j.dst, j.src, j.bytes);
    } else if (j.kind == JOB_F32_TO_F64) {
        const float *s = (const float *)j.src;
        double *d = (double *)j.dst;
        const double sc = j.scale;
        for (size_t i = 0, n = j.bytes / 4; i < n; ++i) d[i] = (double)s[i] * sc;
    } else {
        if (!pack_u8_piece((unsigned char *)j.dst, (const float *)j.src, j.bytes / 4)) j.inexact->store(1, std::memory_order_relaxed);
    }
}

// Persistent host threads that execute job lists in 1 MB pieces (the caller's thread works too).  One core moves
// ~10 GB/s; a full-HD triplet is 71 MB in and 35 MB out, so single-threaded staging would cost several times the
// 1.5 ms the GPU needs for it.
class CopyPool {
public:
    explicit CopyPool(int workers)
    {
        for (int i = 0; i < workers; ++i) th_.emplace_back([this] { worker(); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    int workers() const { return (int)th_.size(); }
    void run(const std::vector<CopyJob> &jobs)
    {
        constexpr size_t kPiece = 1 << 20;
        std::vector<CopyJob> pieces;
        size_t bytes = 0;
        for (const CopyJob &j : jobs) {
            const size_t dmul = j.kind == JOB_F32_TO_F64 ? 2 : 1, ddiv = j.kind == JOB_PACK_U8 ? 4 : 1;
            for (size_t o = 0; o < j.bytes; o += kPiece) {
                CopyJob q = j;
                q.dst = (char *)j.dst + o * dmul / ddiv;
                q.src = (const char *)j.src + o;
                q.bytes = std::min(kPiece, j.bytes - o);
                pieces.push_back(q);
            }
            bytes += j.bytes;
        }
        if (th_.empty() || bytes < (2u << 20)) {
            for (const CopyJob &j : pieces) run_piece(j);
            return;
        }
        std::unique_lock<std::mutex> l(m_);
        pieces_ = &pieces;
        next_ = done_ = 0;
        cv_.notify_all();
        while (next_ < pieces.size()) {
            const CopyJob j = pieces[next_++];
            l.unlock();
            run_piece(j);
            l.lock();
            ++done_;
        }
        cv_done_.wait(l, [&] { return done_ == pieces.size(); });
        pieces_ = nullptr;
    }

private:
    void worker()
    {
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [&] { return stop_ || (pieces_ && next_ < pieces_->size()); });
            if (stop_) return;
            const CopyJob j = (*pieces_)[next_++];
            l.unlock();
            run_piece(j);
            l.lock();
            if (++done_ == pieces_->size()) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    const std::vector<CopyJob> *pieces_ = nullptr;
    size_t next_ = 0, done_ = 0;
    bool stop_ = false;
};

}  // namespace b2f

// A stream (include/b2f.h: b2f_stream_open): the features of the last frames of `cams` cameras, kept on the device between pushes.
// ONE device block of its own, outside the arena and the workspaces of the other entries (those may be re-allocated between two pushes):
//   ring     3 slots x [level 3..7] x [cam]: cs[l] of the frames of a push, chunk-planar; slot of push k = (k - 1) % 3
//   frames   3 slots x [cam]: the frames as the pyramid read them (the caller's bytes / floats at a /64 size, else the normalized
//            scaled frames): the input of the pyramid, and what est[3] of a Hard model warps two pushes later
//   work     the buffers between the input and the outputs of a push (upload / image.scale / the network's outputs / the host
//            entries' outputs), carved once at open for every output a push may ask for
//   raw      B2F_STREAM_WARP at a size that is no multiple of 64 only: 3 slots x [cam] of the caller's frames as pushed (at a /64 size
//            the frame slots hold them): what the warp of a push samples, and the upload target of a host push
//   warp     B2F_STREAM_WARP: the warped neighbours and the photometric records of a host push; B2F_STREAM_PAST: the past flow
// and one page-locked block that stages pageable host buffers.  The pieces of a flag lie behind everything else, so a stream opened
// without flags (b2f_stream_open) has the block it always had.
struct b2f_stream {
    b2f_ctx *ctx = nullptr;
    int cams = 0, in_kind = B2F_IN_UNIT, H0 = 0, W0 = 0;
    long long pushed = 0;          // frames pushed since open / the last reset
    bool broken = false;           // a HIP call failed inside a push: the ring may hold half a frame; reset clears it
    char *dev = nullptr;
    size_t dev_bytes = 0;
    float *lvl[3][8] = {{nullptr}};    // [slot][level]: cams images
    char *frame[3] = {nullptr};        // [slot]: cams frames
    int frame_kind = B2F_IN_UNIT;      // how the forward pass reads a frame slot
    size_t frame_bytes = 0;            // of one slot
    unsigned char *d_u8 = nullptr;     // a rescaled byte stream: the upload, unpacked into d_up
    float *d_up = nullptr, *d_tmp = nullptr;   // a rescaled stream: the frames at H0 x W0 and image.scale's row pass
    float *d_flow = nullptr, *d_occ = nullptr, *d_est3 = nullptr;   // the network's outputs (d_occ: Hard only)
    float *d_flow32 = nullptr, *d_prob = nullptr;   // host pushes: outputs at H0 x W0 (= d_flow / the network's planes without a rescale)
    unsigned char *d_fo = nullptr, *d_bo = nullptr, *d_rgb = nullptr;
    double *d_max = nullptr;
    int flags = 0;                     // B2F_STREAM_* of b2f_stream_open_ex
    char *raw[3] = {nullptr};          // [slot]: cams frames as pushed (B2F_STREAM_WARP at a rescaled size; else null: frame[] holds them)
    size_t raw_bytes = 0;              // of one slot
    void *d_warp = nullptr;            // B2F_STREAM_WARP, host pushes: cams x 2 x 3 x H0 x W0 in the stream's element type ...
    unsigned long long *d_photo = nullptr;   // ... and cams x B2F_PHOTO_WORDS words
    float *d_past = nullptr, *d_past32 = nullptr;   // B2F_STREAM_PAST: skip_ubfs[3] at the network size and at H0 x W0 (= d_past without a rescale)
    char *pin = nullptr;               // staging of pageable host buffers: [frames | flow | occ_prob | masks | rgb | max | warped | photo | past_flow]
    size_t pin_bytes = 0;
};

struct b2f_ctx : b2f::KernelOpts {
    int device = 0;
    bool past_flow = false;
    b2f::GraphOpts g;           // graph shape (createModelMulti options); g.past_flow == past_flow
    long long nparams = 0;
    hipStream_t stream = nullptr;
    std::vector<b2f::ConvDesc> lay;
    std::vector<b2f::PackedConv> packed;
    float *w_dev = nullptr;     // flat canonical weights
    float *wpk_dev = nullptr;   // packed kernel-side copies
    size_t wpk_floats = 0;
    size_t first_w_off = 0, first_b_off = 0;   // [27][16] weights + bias of the first pyramid conv (conv_first_kernel)
    // workspace arena
    float *arena = nullptr;
    size_t arena_floats = 0;
    int wsB = 0, wsH = 0, wsW = 0;
    // options (b2f_set_option: kOptions in b2f_api.hip; those of the kernel choice are the KernelOpts base)
    int use_graph = 0, profile = 0;
    int host_graph = 1;   // b2f_compute_flow*: replay hipGraphs for repeated (shape, sub-batch) combinations
    int cur_batch = 0;             // triplets of the REQUEST the forward pass being issued belongs to (run_conv's per-launch rule for single-triplet calls)
    int req_batch = 0;             // set by the host-buffer entry points to the caller's n while they issue their sub-batches (0: a forward call's own B):
                                   // the kernel choice follows the caller's request, so a triplet's bits do not depend on its position in a batch
    int corr_ablate = 0;           // profiling only, see CorrLaunch::ablate
    int corr_variant = -1;         // warp + cost volume: -1 auto, 0 regular, 1 latency variant (bit-identical results)
    int op_wino_split = 0;         // b2f_op_conv3x3: F(2x2) kernel with one block per 32-output N tile (tests)
    int op_gradw_partials = 0;     // b2f_op_conv3x3[s2]_backward: > 0 cuts the pixels into (at most) this many partial sums instead of the rule's (tests)
    int op_hole_fill = 0;          // b2f_op_layer: the input channels the layer does not read hold 1 + op_hole_fill + slot / 256 (tests)
    int profile_layers = 0;        // one profile row per (layer shape, map size)
    long long host_subbatch_pixels = 16ll << 20;
    int host_threads = 0;          // 0 = auto
    int host_u8 = 1, host_ramp = 1;
    int debug_fail_next = 0;       // tests: the next b2f_compute_flow* call on this context fails (cross-thread error hand-over of b2f_multi_*)
    // tests ("Guards"): neither is seeded from the environment; setting either frees the arena and drops the captured graphs
    int arena_guard = 0;           // floats (a multiple of 64) that make_plan places before the first buffer and after every buffer
    int arena_fill = 0;            // 1: the arena (guards included) and a stream's device block start as kGuardWord instead of 0
    std::vector<b2f::ArenaGuard> guards;   // arena_guard > 0: the guards of the plan the arena was last filled for (b2f_arena_check)
    long long arena_layout[9] = {0};       // arena_guard / arena_fill set: that plan's identity; a pass with another one refills the arena first
    std::map<b2f::GraphKey, hipGraphExec_t> graphs;
    // output table of the generic executor (non-shipped graph shapes), kept between calls of one (B, H, W)
    std::vector<float *> gen_out;
    int genB = 0, genH = 0, genW = 0;
    // profiling
    std::vector<std::string> prof_names;
    std::vector<double> prof_ms;
    std::vector<long long> prof_n;
    std::vector<b2f::ProfEvent> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    // host-buffer pipeline (b2f_compute_flow_batch)
    hipStream_t s_in = nullptr, s_out = nullptr;
    b2f::HostSlot slot[2];
    std::unique_ptr<b2f::CopyPool> pool_in, pool_out;
    b2f::DevWork dwork;           // b2f_compute_flow_device / b2f_compute_flow_sequence_device
    b2f::DevWork vis_max;         // b2f_flow_rgb_device without dev_max_used: the per-image maxima of the automatic mode
    b2f::DevWork loss_pyr;        // b2f_table_loss_device / b2f_forward_loss*: the pooled reference images R_1 .. R_{L-1} (test.lua:266-297)
    b2f::DevWork loss_work;       // b2f_forward_loss*: [input | output table | records] of a sub-batch
    b2f::DevWork loss_rec;        // the *_grad_ssim / *_grad_plain entries without records: n x L x 32 / 40 words for the ranges (table_loss_grad_run)
    std::vector<b2f_stream *> streams;   // open streams (b2f_stream_open); b2f_destroy closes what is left
    // arena_guard on a non-shipped graph: the generic executor's buffers of the layout in arena_layout; guards[].name points into their names
    std::vector<b2f::GraphBuf> graph_bufs;
};

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return b2f::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)
// function-try-block tail of every int-returning entry point: nothing is thrown across the C ABI
#define B2F_CATCH(fn_)                                                                        \
    catch (const std::exception &e_) { return b2f::api_fail(std::string(fn_ ": ") + e_.what()); } \
    catch (...) { return b2f::api_fail(fn_ ": unknown exception"); }
#define CHK(expr)                         \
    do {                                  \
        int rc_ = (expr);                 \
        if (rc_ != 0) return rc_;         \
    } while (0)

namespace b2f {
// b2f_api.hip
int check_shape(int B, int H, int W);
// profile = 1: brackets a launch made outside b2f_api.hip with events on s, as a row `name` of b2f_profile_read (false: profiling is off)
bool prof_open(b2f_ctx *c, hipStream_t s, const char *name, ProfEvent *pe);
void prof_close(b2f_ctx *c, hipStream_t s, const ProfEvent &pe);
void drop_graphs(b2f_ctx *c);
// b2f_tableloss.hip: grows a workspace of the context to `bytes` (after a device synchronisation when it has to be replaced)
int ensure_dev_work(DevWork &dw, size_t bytes);
void drop_gen_out(b2f_ctx *c);
// model:forward on device pointers, optionally replayed from a hipGraph (see b2f_api.hip); seq: dev_in holds the B + 2 frames
// of a sequence (T x 3 x H x W) instead of B triplets (B x 9 x H x W)
// sp: a push of a stream -- dev_in holds its B = cams frames (see StreamPass)
// dev_past: the past flow skip_ubfs[3] (B x 2 x H x W); runs the past-flow decoder chain, refused on a model without one
int forward_device(b2f_ctx *c, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow, float *dev_occ,
                   float *dev_est3, hipStream_t s, bool graph, bool seq = false, const StreamPass *sp = nullptr, float *dev_past = nullptr);
// b2f_pipeline.hip: the checks of a request that need no context and no HIP call (in_kind, T / n, shape, required pointers); 0 = fine
int check_request(const FlowRequest &r);
// b2f_pipeline.hip: a request on host buffers (the upload / kernels / download pipeline) and on device buffers (the kernels alone,
// asynchronous on `stream`, nullptr: the context's)
int compute_flow_host(b2f_ctx *c, const FlowRequest &r);
// b2f_api.hip: what the HIP runtime knows of p: -1 device (managed, array) memory, 1 page-locked host memory, 0 anything else, which is
// pageable host memory
int pointer_kind(const void *p);
inline bool host_memory(const void *p) { return pointer_kind(p) >= 0; }
// b2f_api.hip: the pointer checks of the device entry w, null pointers skipped: all 16-byte aligned, then the context (null: refused
// here, for the entries that have not looked yet) and hipSetDevice, then none of them host memory -- "(use <use>)" names the entries for that
// aligned: so many of them, the first ones, have to be (byte planes need not)
int check_device_pointers(const std::string &w, const b2f_ctx *c, const char *use, const void *const *ptrs, size_t count, size_t aligned);
inline int check_device_pointers(const std::string &w, const b2f_ctx *c, const char *use, std::initializer_list<const void *> ptrs)
{
    return check_device_pointers(w, c, use, ptrs.begin(), ptrs.size(), ptrs.size());
}

// ---- the table-loss family ----
// The objective of a table-loss entry: the records of test.lua:266-297 alone (B2F_LOSS_WORDS), with the fine-tuning terms of
// README.md:89-102 behind them (B2F_LOSS_FT_WORDS), with the SSIM + L1 sums of OSSIML1Criterion.lua and their range (B2F_LOSS_SSIM_WORDS),
// with the photometric sums without occlusion masking of MBCCriterion.lua / MSSIML1Criterion.lua and their range (B2F_LOSS_PLAIN_WORDS),
// or the supervised objective of train.lua:296-334 (B2F_LOSS_EPE_WORDS)
enum LossObjective { kLossPme = 0, kLossFt = 1, kLossSsim = 2, kLossPlain = 3, kLossEpe = 4 };

// Which objective and which outputs: what every layer of the family takes, from the extern "C" one-liner that builds it (loss_records,
// loss_grad, loss_epe below) down to the launchers' callers.  The first part is what the entry was given; resolve() checks it and fills
// the second part.  The four unsupervised objectives require the records in their plain entries and the gradient table in their *_grad*
// entries (grad_entry), where the forward entries take the records too; the supervised one takes either or both everywhere.
struct LossSpec {
    LossObjective obj = kLossPme;
    bool grad_entry = false;
    // opts: b2f_loss_grad_opts / _ft_opts / _ssim_opts / _plain_opts of a *_grad* entry by obj, b2f_loss_epe_opts of kLossEpe; nullptr:
    // the defaults
    const void *opts = nullptr;
    int range_mode = 0;              // kLossSsim, kLossPlain: B2F_SSIM_RANGE_*, and L x 2 host floats with B2F_SSIM_RANGE_GIVEN
    const float *ranges = nullptr;
    // kLossEpe: the ground truth of image 0 (valid and gt_occ may be null), host or device memory as the entry has it; B2F_EPE_COUNT_*
    // and L x 2 host doubles with B2F_EPE_COUNT_GIVEN
    const float *gt_flow = nullptr;
    const unsigned char *valid = nullptr, *gt_occ = nullptr;
    int count_mode = 0;
    const double *counts = nullptr;
    // resolved: the first-order fields and smooth_second_order of every *_grad* kind in o (pme: both flags 0; ssim, plain: pme_criterion 0,
    // unused), the rest of ssim and plain beside it; the options of kLossEpe
    b2f_loss_grad_ft_opts o = {};
    double ssim_alpha = 0.0;
    int plain_criterion = 0, plain_penalty = 0;   // B2F_PLAIN_*
    b2f_loss_epe_opts epe = {};

    bool is_epe() const { return obj == kLossEpe; }
    bool ranged() const { return obj == kLossSsim || obj == kLossPlain; }   // range_mode and ranges are read
    int words() const   // of a record
    {
        static const int kWords[5] = {B2F_LOSS_WORDS, B2F_LOSS_FT_WORDS, B2F_LOSS_SSIM_WORDS, B2F_LOSS_PLAIN_WORDS, B2F_LOSS_EPE_WORDS};
        return kWords[obj];
    }
    // b2f_table_loss<suffix>_device, b2f_forward_loss<suffix>, ...
    const char *suffix() const
    {
        static const char *const kSuffix[2][5] = {{"", "_ft", "_ssim", "_plain", "_epe"}, {"_grad", "_grad_ft", "_grad_ssim", "_grad_plain", "_epe"}};
        return kSuffix[grad_entry][obj];
    }
    // the rows of b2f_profile_read behind table_loss (and table_loss_range): of the kernel that adds an objective's words to the
    // records (nullptr: pme has none) and of the gradient table's kernels; kLossEpe has the one row for both
    const char *terms_row() const
    {
        static const char *const kRow[5] = {nullptr, "table_loss_ft", "table_loss_ssim", "table_loss_plain", "table_loss_epe"};
        return kRow[obj];
    }
    const char *grad_row() const
    {
        static const char *const kRow[5] = {"table_loss_grad", "table_loss_grad_ft", "table_loss_grad_ssim", "table_loss_grad_plain", "table_loss_epe"};
        return kRow[obj];
    }
    // the entries a device entry points a caller with host memory to
    const char *host_entries() const
    {
        static const char *const kRecords = "b2f_op_table_loss / b2f_table_loss_host", *const kEpe = "b2f_op_table_loss_epe / b2f_table_loss_epe_host";
        static const char *const kUse[2][5] = {{kRecords, kRecords, kRecords, kRecords, kEpe},
                                               {"b2f_op_table_loss_grad / b2f_table_loss_grad_host", "b2f_op_table_loss_grad_ft / b2f_table_loss_grad_ft_host",
                                                "b2f_op_table_loss_grad_ssim / b2f_table_loss_grad_ssim_host",
                                                "b2f_op_table_loss_grad_plain / b2f_table_loss_grad_plain_host", kEpe}};
        return kUse[grad_entry][obj];
    }
    // nullptr, or why these outputs are refused
    const char *outputs_refusal(const void *loss, const void *grad) const
    {
        if (is_epe()) return !loss && !grad ? "loss and grad are both null: nothing to compute" : nullptr;
        return (grad_entry ? !grad : !loss) ? "null argument" : nullptr;
    }
    // b2f_tableloss.hip: nullptr, or why the range is refused; nullptr and the second part filled (the defaults where opts is null), or why
    // the options, then the range, or the ground truth and the counts of a table of L levels, are refused, as include/b2f.h says
    const char *range_refusal() const;
    const char *resolve(int L);
    // nullptr, or why a table entry with a context refuses this objective on its model: a two_frame model has no occlusions in its table
    // (MBCCriterion.lua:39-42: the tensors of a level shift, and the table has none of the words 0 .. 15)
    const char *model_refusal(const b2f_ctx *c) const
    {
        if (!c->g.two_frame) return nullptr;
        return obj == kLossPlain ? "a two_frame model has no occlusions in its table; the *_plain entries are not defined for it"
               : is_epe()        ? "a two_frame model has no occlusions in its table; the table loss is not defined for it"
                                 : nullptr;
    }
    // nullptr, or why a request that is split over several GPUs refuses this (a shard's batch range, or its counts, would depend on the split)
    const char *sharded_refusal() const
    {
        if (ranged() && range_mode == B2F_SSIM_RANGE_BATCH)
            return "B2F_SSIM_RANGE_BATCH is not served over several GPUs: the images of a request are split; use B2F_SSIM_RANGE_IMAGE or "
                   "B2F_SSIM_RANGE_GIVEN";
        if (is_epe() && count_mode == B2F_EPE_COUNT_BATCH)
            return "B2F_EPE_COUNT_BATCH is not served over several GPUs: the images of a request are split; use B2F_EPE_COUNT_IMAGE or "
                   "B2F_EPE_COUNT_GIVEN";
        return nullptr;
    }
    // the same for the images from `image` on of a request of H x W = hw pixels: the ground truth moves on, on the host and on the device alike
    LossSpec at_image(size_t image, size_t hw) const
    {
        LossSpec d = *this;
        if (gt_flow) d.gt_flow = gt_flow + image * 2 * hw;
        if (valid) d.valid = valid + image * hw;
        if (gt_occ) d.gt_occ = gt_occ + image * hw;
        return d;
    }
};
inline LossSpec loss_spec(LossObjective obj, bool grad_entry, const void *opts, int range_mode, const float *ranges)
{
    LossSpec d;
    d.obj = obj; d.grad_entry = grad_entry; d.opts = opts; d.range_mode = range_mode; d.ranges = ranges;
    return d;
}
inline LossSpec loss_records(LossObjective obj, int range_mode = 0, const float *ranges = nullptr) { return loss_spec(obj, false, nullptr, range_mode, ranges); }
inline LossSpec loss_grad(const b2f_loss_grad_opts *o) { return loss_spec(kLossPme, true, o, 0, nullptr); }
inline LossSpec loss_grad(const b2f_loss_grad_ft_opts *o) { return loss_spec(kLossFt, true, o, 0, nullptr); }
inline LossSpec loss_grad(const b2f_loss_grad_ssim_opts *o, int range_mode, const float *ranges) { return loss_spec(kLossSsim, true, o, range_mode, ranges); }
inline LossSpec loss_grad(const b2f_loss_grad_plain_opts *o, int range_mode, const float *ranges) { return loss_spec(kLossPlain, true, o, range_mode, ranges); }
inline LossSpec loss_epe(const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ, const b2f_loss_epe_opts *o, int count_mode,
                         const double *counts)
{
    LossSpec d = loss_spec(kLossEpe, false, o, 0, nullptr);
    d.gt_flow = gt_flow; d.valid = valid; d.gt_occ = gt_occ; d.count_mode = count_mode; d.counts = counts;
    return d;
}

// b2f_tableloss.hip: tensors per level of a table of n_outs tensors on this context: its own kind where that divides n_outs, else the
// other one; 0: neither (kTableSizeRefusal)
int level_size(const b2f_ctx *c, int n_outs);
// b2f_tableloss.hip: what every entry on a table checks without a HIP call, for all five objectives: the outputs asked for, the shape
// (table_loss_refusal, into *L), null tensors, d.resolve, and that no output -- loss (or null), the gradient table (or null) -- is an
// input or another output.  per: tensors per level; ref is not read by kLossEpe
int check_table(const std::string &w, LossSpec &d, const float *const *table, float *const *grad, const unsigned long long *loss, const float *ref, int n_outs,
                int per, int n, int H, int W, double flow_scale, int *L);
// b2f_tableloss.hip: the one body behind b2f_table_loss*_device, b2f_table_loss_grad*_device and b2f_table_loss_epe_device, and the one
// behind the b2f_op_table_loss* entries, which stages host tensors in a guarded OpStage and calls the former
int table_loss_device(const std::string &w, LossSpec d, b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                      double flow_scale, unsigned long long *dev_loss, float *const *dev_grad, void *stream);
int table_loss_op(const std::string &w, LossSpec d, b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                  double flow_scale, unsigned long long *loss, float *const *grad);
// b2f_tableloss.hip: the one body behind the b2f_table_loss*_host entries: check_table, then the objective's implementation on the CPU
// (b2f_host.cpp); rescale: kLossEpe's
int table_loss_host_entry(const std::string &w, LossSpec d, const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                          double flow_scale, unsigned long long *loss, float *const *grad, int rescale = 0);
// b2f_tableloss.hip: records and / or gradient table of n images of a resolved d on s, by one of the three below: kLossEpe by
// table_loss_epe_run; else the records, where asked for, by table_loss_run and then the gradient table, where asked for, by
// table_loss_grad_run, which finds the pyramid (and the ranges) the records' launch has left
int table_loss_dispatch(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, unsigned long long *dev_loss, const LossSpec &d, int L,
                        bool past, int n, int H, int W, const float *dev_ref, size_t ref_stride, double flow_scale);
// b2f_tableloss.hip: the records of test.lua:266-297 of n images on s, under the profile row table_loss; then, by d.obj, the fine-tuning
// terms behind them (table_loss_ft), the ranges and the SSIM + L1 sums (table_loss_range, table_loss_ssim) or the ranges and the sums
// without occlusion masking (table_loss_range, table_loss_plain).  Builds R_1 .. R_{L-1} in c->loss_pyr first.
int table_loss_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, int L, bool past, int n, int H, int W, const float *dev_ref,
                   size_t ref_stride, double flow_scale, unsigned long long *dev_loss, const LossSpec &d);
// b2f_tableloss.hip: the gradient table of train.lua:428-468 of n images on s, from a resolved d; dev_loss: the records
// table_loss_run(.., d) has written on s with R_1 .. R_{L-1}, or nullptr: the pyramid is built first, and where the objective reads
// them the ranges into a zeroed record buffer of the context (c->loss_rec)
int table_loss_grad_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, int L, bool past, int n, int H, int W,
                        const float *dev_ref, size_t ref_stride, double flow_scale, const LossSpec &d, unsigned long long *dev_loss);
// b2f_tableloss_epe.hip: the records (dev_loss, or nullptr) and / or the gradient table (dev_grad, or nullptr) of the supervised objective
// of train.lua:296-334 of n images on s, from a resolved d whose ground truth is device memory, under the profile row table_loss_epe;
// rescale is the context's rescale_flow; the counting pass of size_average goes into c->loss_rec
int table_loss_epe_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, int L, bool past, int n, int H, int W,
                       double flow_scale, const LossSpec &d, unsigned long long *dev_loss);
// b2f_api.hip: model:forward and the objective d on n of a request of `req` triplets (0: n) from host memory -- the b2f_forward_loss*
// entries of every objective, and a shard of b2f_multi_forward_loss*, which passes the caller's n down as req.  loss, grad and outs as
// d.outputs_refusal has them; n_outs counts grad, and outs where there is no grad.
int forward_loss_host(b2f_ctx *c, const float *x, int n, int req, int H, int W, double flow_scale, LossSpec d, unsigned long long *loss, float *const *grad,
                      int n_outs, float *const *outs);
int compute_flow_device(b2f_ctx *c, const FlowRequest &r, void *stream);
// b2f_pipeline.hip: a push (r.stream) on host buffers, synchronous, and on device buffers, asynchronous on `stream`; *ready = 1 when
// the outputs were written (from the third push on)
int stream_push_host(const FlowRequest &r, int *ready);
int stream_push_device(const FlowRequest &r, void *stream, int *ready);
// pieces of b2f_api.hip the generic graph executor (b2f_graph.hip) and the kernel test entries (b2f_ops.hip) build on
ConvSeg cp8_seg(const float *ptr, int C, size_t hw);
int find_conv_id(const b2f_ctx *c, int kind, int level, int idx);
int run_conv_layer(b2f_ctx *c, hipStream_t s, bool cap, int conv_id, const ConvSeg *segs, int nimg, int H, int W, int stride, int leaky,
                   float *out);
// the conv table as b2f_op_conv3x3 and b2f_op_layer use it (b2f_api.hip, "the conv kernels" and launch_layer)
ConvKernel base_kernel(int ci, int co, bool stride1, bool two_segments);
void place_packings(PackedConv &p, bool stride1, const KernelOpts &o, size_t *total);
void fill_packings(const PackedConv &p, const float *w, const float *b, int ci, const int *cin_map, float *host);
std::vector<int> layer_cin_map(const ConvDesc &d, bool shipped, PackedConv &p);
int launch_layer(b2f_ctx *c, hipStream_t s, bool prof, const PackedConv &p, const float *wpk, const KernelOpts &o, int cur_batch, ConvLaunch &L);
// b2f_ops.hip: the first pyramid conv's weights, Torch 16 x 3 x 3 x 3, as conv_first_kernel reads them: [tap (c, ky, kx)][cout]
void pack_first_conv(const float *w, float *wp);
// the arena for a pass of the generic executor over `floats` floats laid out as `bufs` (empty without arena_guard) for shape B x H x W
int ensure_arena(b2f_ctx *c, size_t floats, std::vector<GraphBuf> &&bufs, int B, int H, int W);
// b2f_graph.hip: model:forward for the non-shipped graph shapes; outs = the whole output table (planar device buffers)
int graph_forward(b2f_ctx *c, hipStream_t s, bool cap, const void *dev_in, int in_kind, int B, int H, int W, float *const *outs);
}  // namespace b2f
