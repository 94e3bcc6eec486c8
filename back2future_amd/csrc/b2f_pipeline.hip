// The computeFlow boundary of libb2f.so (back2future.lua:47-95): every b2f_compute_flow* entry point (and b2f_multi's, b2f_multi.hip)
// builds one FlowRequest.  check_request() refuses a malformed one before any HIP call; compute_flow_host() runs it on host buffers as a
// double-buffered upload / kernels / download pipeline around model:forward, compute_flow_device() runs the kernels half alone on
// device buffers.  Both cut the request with plan_subbatches() and run every sub-batch through run_kernels().  Device kernels of the
// pre/post processing: b2f_boundary.hip.
#include "b2f_ctx.h"

#include <cstdlib>

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace {

// 1 when [p, p + bytes) is page-locked host memory known to the HIP runtime (hipHostMalloc / hipHostRegister, e.g. a
// torch pin_memory() tensor): such buffers are DMA'd directly; 0 for ordinary (pageable) host memory, which goes
// through the pinned slot; -1 for device / managed memory, which the host entry points refuse
int mem_kind(const void *p, size_t bytes)
{
    int kind = 1;
    for (const char *q : {(const char *)p, (const char *)p + bytes - 1}) {
        const int k = pointer_kind(q);
        if (k < 0) return -1;
        kind = std::min(kind, k);
    }
    return kind;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// what a slot holds beyond the f64 path's buffers
struct SlotNeeds {
    bool same, stage_in, stage_masks, use_u8;
    bool occ_net;      // d_occ: skip_occs[3] of a Hard model (f32 path with occ_prob)
    bool prob;         // d_prob: occ_prob at H0 x W0 (f32 path with occ_prob and a rescale)
    bool stage_flow;   // h_flow32: the f64 path always, the f32 path for a pageable flow buffer
    bool stage_prob;   // h_prob: pageable occ_prob buffer
    bool rgb;          // d_rgb, d_max: an rgb request
    bool stage_rgb;    // h_rgb: pageable rgb buffer
    bool stage_max;    // h_max: pageable max_used buffer
    bool score;        // d_gt, d_score: a score request
    bool valid, gtocc; // d_valid, d_gtocc: the optional byte planes of the ground truth
    bool stage_gt, stage_valid, stage_gtocc, stage_score;   // h_gt, h_valid, h_gtocc, h_score: pageable buffers
    size_t warp_esz;   // d_warp: the warped neighbours of a warp request, bytes per sample (0: not asked for)
    bool photo;        // d_photo: its photometric records
    bool stage_warp, stage_photo;   // h_warp, h_photo: pageable buffers
    bool past;         // d_past, d_past32: a request with the past flow (FlowOutputs::want_past)
    bool stage_past;   // h_past: pageable past_flow buffer
};

// carve the slot's device and pinned blobs for sub-batches of up to SB triplets; grows (never shrinks) the blobs
int ensure_slot(b2f_ctx *c, HostSlot &hs, int SB, size_t hw0, size_t hw, int H0, int fw, int C3, const SlotNeeds &q)
{
    const bool same = q.same;
    const size_t n_up = align256((size_t)SB * 9 * hw0 * 4), n_u8 = q.use_u8 ? align256((size_t)SB * 9 * hw0) : 0,
                 n_in = same ? 0 : align256((size_t)SB * 9 * hw * 4), n_tmp = same ? 0 : align256((size_t)SB * 9 * H0 * fw * 4),
                 n_flow = align256((size_t)SB * 2 * hw * 4), n_est3 = align256((size_t)SB * C3 * hw * 4),
                 n_f32 = align256((size_t)SB * 2 * hw0 * 4), n_occ = align256((size_t)SB * hw0);
    const size_t n_onet = q.occ_net ? n_flow : 0, n_prob = q.prob ? n_f32 : 0;
    const size_t n_rgb = q.rgb ? align256((size_t)SB * 3 * hw0) : 0, n_max = q.rgb ? align256((size_t)SB * sizeof(double)) : 0;
    const size_t n_gt = q.score ? n_f32 : 0, n_va = q.valid ? n_occ : 0, n_lb = q.gtocc ? n_occ : 0,
                 n_sc = q.score ? align256((size_t)SB * B2F_SCORE_WORDS * sizeof(unsigned long long)) : 0;
    const size_t n_wp = align256((size_t)SB * 6 * hw0 * q.warp_esz),
                 n_ph = q.photo ? align256((size_t)SB * B2F_PHOTO_WORDS * sizeof(unsigned long long)) : 0;
    const size_t n_pnet = q.past ? n_flow : 0, n_p32 = (q.past && !same) ? n_f32 : 0;
    const size_t need_dev = n_up + n_u8 + n_in + n_tmp + n_flow + n_est3 + (same ? 0 : n_f32) + n_onet + n_prob + 2 * n_occ + n_rgb + n_max +
                            n_gt + n_va + n_lb + n_sc + n_wp + n_ph + n_pnet + n_p32;
    if (need_dev > hs.dev_bytes) {
        if (hs.dev) {
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipFree(hs.dev));
            hs.dev = nullptr; hs.dev_bytes = 0;
            drop_graphs(c);   // graphs are keyed on slot pointers
        }
        HIPCHK(hipMalloc(&hs.dev, need_dev));
        hs.dev_bytes = need_dev;
    }
    char *d = hs.dev;
    hs.d_up = (float *)d; d += n_up;
    hs.d_u8 = (unsigned char *)d; d += n_u8;
    hs.d_in = same ? hs.d_up : (float *)d; d += n_in;
    hs.d_tmp = (float *)d; d += n_tmp;
    hs.d_flow = (float *)d; d += n_flow;
    hs.d_est3 = (float *)d; d += n_est3;
    hs.d_flow32 = same ? hs.d_flow : (float *)d; d += same ? 0 : n_f32;
    hs.d_occ = q.occ_net ? (float *)d : nullptr; d += n_onet;
    hs.d_prob = q.prob ? (float *)d : nullptr; d += n_prob;
    hs.d_fo = (unsigned char *)d; d += n_occ;
    hs.d_bo = (unsigned char *)d; d += n_occ;
    hs.d_rgb = q.rgb ? (unsigned char *)d : nullptr; d += n_rgb;
    hs.d_max = q.rgb ? (double *)d : nullptr; d += n_max;
    hs.d_gt = q.score ? (float *)d : nullptr; d += n_gt;
    hs.d_valid = q.valid ? (unsigned char *)d : nullptr; d += n_va;
    hs.d_gtocc = q.gtocc ? (unsigned char *)d : nullptr; d += n_lb;
    hs.d_score = q.score ? (unsigned long long *)d : nullptr; d += n_sc;
    hs.d_warp = q.warp_esz ? (void *)d : nullptr; d += n_wp;
    hs.d_photo = q.photo ? (unsigned long long *)d : nullptr; d += n_ph;
    hs.d_past = q.past ? (float *)d : nullptr; d += n_pnet;
    hs.d_past32 = !q.past ? nullptr : same ? hs.d_past : (float *)d;
    const size_t n_hf = q.stage_flow ? n_f32 : 0, n_hp = q.stage_prob ? n_f32 : 0;
    const size_t n_hr = q.stage_rgb ? n_rgb : 0, n_hm = q.stage_max ? n_max : 0;
    const size_t n_hg = q.stage_gt ? n_gt : 0, n_hv = q.stage_valid ? n_va : 0, n_hl = q.stage_gtocc ? n_lb : 0, n_hs = q.stage_score ? n_sc : 0;
    const size_t n_hw = q.stage_warp ? n_wp : 0, n_hph = q.stage_photo ? n_ph : 0, n_hpa = q.stage_past ? n_f32 : 0;
    const size_t need_pin = (q.stage_in ? n_up : 0) + n_u8 + n_hf + n_hp + (q.stage_masks ? 2 * n_occ : 0) + n_hr + n_hm + n_hg + n_hv + n_hl + n_hs +
                            n_hw + n_hph + n_hpa;
    if (need_pin > hs.pin_bytes) {
        if (hs.pin) {
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipHostFree(hs.pin));
            hs.pin = nullptr; hs.pin_bytes = 0;
        }
        HIPCHK(hipHostMalloc(&hs.pin, need_pin, hipHostMallocDefault));
        hs.pin_bytes = need_pin;
    }
    char *h = hs.pin;
    hs.h_in = (float *)h; h += q.stage_in ? n_up : 0;
    hs.h_u8 = (unsigned char *)h; h += n_u8;
    hs.h_flow32 = (float *)h; h += n_hf;
    hs.h_prob = (float *)h; h += n_hp;
    hs.h_fo = (unsigned char *)h; h += q.stage_masks ? n_occ : 0;
    hs.h_bo = (unsigned char *)h; h += q.stage_masks ? n_occ : 0;
    hs.h_rgb = (unsigned char *)h; h += n_hr;
    hs.h_max = (double *)h; h += n_hm;
    hs.h_gt = (float *)h; h += n_hg;
    hs.h_valid = (unsigned char *)h; h += n_hv;
    hs.h_gtocc = (unsigned char *)h; h += n_hl;
    hs.h_score = (unsigned long long *)h; h += n_hs;
    hs.h_warp = (void *)h; h += n_hw;
    hs.h_photo = (unsigned long long *)h; h += n_hph;
    hs.h_past = (float *)h;
    for (hipEvent_t *e : {&hs.ev_in, &hs.ev_comp, &hs.ev_out})
        if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return 0;
}

// The sizes of a request: the network runs at fh x fw, H0 x W0 cut down to multiples of 64 (back2future.lua:54-67), and its flow is
// rescaled to H0 x W0 by sc_w / sc_h (:78-79).  C3: channels of est[3].
struct Geometry {
    int H0, W0, fh, fw, C3;
    bool same;        // H0 x W0 is the network size: no image.scale, the outputs are not rescaled
    size_t hw0, hw;   // pixels of an input plane / of a network plane
    double sc_w, sc_h;
};

Geometry geometry(const b2f_ctx *c, int H0, int W0)
{
    const int fw = W0 - W0 % 64, fh = H0 - H0 % 64;
    return {H0, W0, fh, fw, c->past_flow ? 2 : 3, fw == W0 && fh == H0, (size_t)H0 * W0, (size_t)fh * fw, (double)W0 / (double)fw,
            (double)H0 / (double)fh};
}

// The n triplets of a request cut into sub-batches of up to host_subbatch_pixels input pixels per plane set, counted in units: triplets,
// or frames in sequence mode, where a sub-batch also holds the two frames it shares with the next one (and at least the 3 of one
// triplet).  With ramp the sizes start at ~2 Mpx (one full-HD unit) and double up to the largest: the host pipeline's kernels start
// after a small upload instead of a whole sub-batch's.  (first triplet, count) per sub-batch; *SB = triplets of the largest.
std::vector<std::pair<int, int>> plan_subbatches(const b2f_ctx *c, int n, bool seq, size_t hw0, bool ramp, int *SB)
{
    const int gu = seq ? 2 : 0;   // units a sub-batch holds beyond its triplets
    const int SBU = (int)std::min<long long>(n + gu, std::max<long long>(1 + gu, c->host_subbatch_pixels / (long long)hw0));
    const int sz0 = ramp ? (int)std::min<long long>(SBU, std::max<long long>(1 + gu, (2ll << 20) / (long long)hw0)) : SBU;
    std::vector<std::pair<int, int>> subs;
    for (int b0 = 0, sz = sz0; b0 < n; sz = std::min(2 * sz, SBU)) {
        const int nb = std::min(sz - gu, n - b0);
        subs.push_back({b0, nb});
        b0 += nb;
    }
    *SB = SBU - gu;
    return subs;
}

// While it lives, the kernel choice of every sub-batch follows the request's n (a single-triplet request takes the per-launch rule, a
// batch the map-size rule -- for ALL its sub-batches, also those of one triplet the ramp and the tail produce)
struct ReqBatch {
    b2f_ctx *c;
    ReqBatch(b2f_ctx *cc, const FlowRequest &r) : c(cc) { c->req_batch = r.req > 0 ? r.req : r.n; }
    ~ReqBatch() { c->req_batch = 0; }
};

// device buffers of a sub-batch between its input and its outputs
struct NetBuffers {
    float *tmp, *scaled;        // image.scale's row pass and result (unused at the network size)
    float *flow, *occ, *est3;   // the forward pass's outputs at fh x fw; occ: skip_occs[3] of a Hard model, nullptr when not needed
    float *past = nullptr;      // skip_ubfs[3] at fh x fw: set when the request wants the past flow (the pass then runs the past chain)
};

// The kernels of a sub-batch of nb triplets on s.  x: its `planes` input planes at H0 x W0, B2F_IN_UNIT floats or, at the network
// size only, B2F_IN_U8 bytes.  ColorNormalize, then image.scale to the /64 size (:50-71) -- without a rescale the raw planes go to the
// network as they are and the first conv kernel normalizes on the fly --, the forward pass, and outputs_f32_kernel into `out` (device
// buffers at H0 x W0; nullptr: not written).  The flow of an f64 request is left unscaled: the host threads form `double * sc` (:80-84).
// out.rgb: the pictures of that f32 flow (xy2rgb, b2f_vis.hip), read from out.flow32 or, at the network size, from net.flow itself.
// out.scores: the records of that f32 flow and occ_prob against out.gt_flow / valid / gt_occ (device copies; b2f_score.hip), read like the
// pictures' flow: from out.flow32 / out.occ_prob or, at the network size, from the network's own planes.
// out.warped / out.photo: the motion-compensated neighbours and their photometric records (b2f_warp.hip) of that f32 flow and occ_prob,
// chosen like the scores' inputs, and of the sub-batch's own frames: x as it came in, before image.scale replaces it, triplet b's
// three frames 9 planes apart, or the frames of a sequence 3 planes apart.
// net.past / out.past32: the past flow of a Soft model, rescaled by a second launch of outputs_f32_kernel on its planes (the launch
// that writes the flow, the probabilities and the masks is the one of a request without it); with out.own_past the warp places the
// past frame's samples with it, read like the flow: from out.past32 or, at the network size, from net.past.
// sp: a push of a stream -- the nb = cams frames go through the pyramid into the ring (net.scaled, where image.scale writes, is their
// frame slot); the rest runs, and the outputs are written, only from the third push on.  Its warp samples the frames of three pushes:
// sp->raw_past / raw_ref / raw_fut, camera b's frames 3 planes apart.
int run_kernels(b2f_ctx *c, const FlowRequest &r, const Geometry &g, const void *x, int kind, long planes, int nb, const NetBuffers &net,
                const FlowOutputs &out, bool graph, hipStream_t s, const StreamPass *sp = nullptr)
{
    const void *frames = x;   // the caller's frames at H0 x W0 and their kind: what a warp request samples
    const int frames_kind = kind;
    if (!g.same) {
        HIPCHK(launch_image_scale((const float *)x, 1, planes, g.H0, g.W0, net.tmp, net.scaled, g.fh, g.fw, s));
        x = net.scaled;
        kind = B2F_IN_NORMALIZED;
    }
    CHK(forward_device(c, x, kind, nb, g.fh, g.fw, net.flow, net.occ, net.est3, s, graph, r.seq, sp, net.past));
    if (sp && !sp->ready) return 0;
    const bool f32 = r.o.f32();
    HIPCHK(launch_outputs_f32(net.flow, g.C3 == 3 ? net.occ : net.est3, net.est3, g.C3, nb, g.fh, g.fw, g.H0, g.W0, f32 ? g.sc_w : 1.0,
                              f32 ? g.sc_h : 1.0, out.flow32, out.occ_prob, out.fwd_occ, out.bwd_occ, s));
    if (out.past32)
        HIPCHK(launch_outputs_f32(net.past, nullptr, nullptr, g.C3, nb, g.fh, g.fw, g.H0, g.W0, g.sc_w, g.sc_h, out.past32, nullptr, nullptr, nullptr, s));
    if (out.rgb) {
        if (!out.flow32 && !g.same) return fail(std::string(r.who) + ": a picture of a rescaled flow needs the flow buffer");
        HIPCHK(launch_flow_rgb(out.flow32 ? out.flow32 : net.flow, nb, g.H0, g.W0, out.max_norm, out.rgb_layout, out.rgb, out.rgb_max, s));
    }
    if (out.scores) {
        const bool want_occ = out.gt_occ != nullptr;
        if (!g.same && (!out.flow32 || (want_occ && !out.occ_prob)))
            return fail(std::string(r.who) + ": the score of a rescaled flow needs the flow and occ_prob buffers");
        const float *prob = !want_occ ? nullptr : g.same ? (g.C3 == 3 ? net.occ : net.est3) : out.occ_prob;
        if (want_occ && !prob) return fail(std::string(r.who) + ": the occlusion scores need skip_occs[3]");
        ProfEvent pe;
        const bool timed = prof_open(c, s, "flow_score", &pe);
        const hipError_t e = launch_flow_score(out.flow32 ? out.flow32 : net.flow, prob, nb, g.H0, g.W0, out.flow_scale, out.gt_flow, out.valid,
                                               out.gt_occ, out.scores, s);
        if (timed) prof_close(c, s, pe);
        HIPCHK(e);
    }
    if (out.warped || out.photo) {
        if (!g.same && (!out.flow32 || (out.photo && !out.occ_prob)))
            return fail(std::string(r.who) + ": the warp of a rescaled flow needs the flow and occ_prob buffers");
        const float *prob = !out.photo ? nullptr : g.same ? (g.C3 == 3 ? net.occ : net.est3) : out.occ_prob;
        if (out.photo && !prob) return fail(std::string(r.who) + ": the photometric record needs skip_occs[3]");
        const float *own_past = !out.own_past ? nullptr : g.same ? net.past : out.past32;
        if (out.own_past && !own_past) return fail(std::string(r.who) + ": the warp with the model's own past flow needs the past-flow buffer");
        if (sp && (!sp->raw_past || !sp->raw_ref || !sp->raw_fut)) return fail(std::string(r.who) + ": the stream keeps no frames for the warp");
        const int wkind = sp ? sp->raw_kind : frames_kind;
        const size_t esz = wkind == B2F_IN_U8 ? 1 : 4, stride = ((r.seq || sp) ? 3 : 9) * g.hw0;
        const char *f0 = (const char *)frames;
        const void *w1 = sp ? sp->raw_past : f0, *w2 = sp ? sp->raw_ref : f0 + 3 * g.hw0 * esz, *w3 = sp ? sp->raw_fut : f0 + 6 * g.hw0 * esz;
        ProfEvent pe;
        const bool timed = prof_open(c, s, "flow_warp", &pe);
        const hipError_t e = launch_flow_warp(out.flow32 ? out.flow32 : net.flow, prob, nb, g.H0, g.W0, out.flow_scale, w1, w2, w3, stride, wkind,
                                              out.warped, out.warped_kind, out.photo, s, own_past);
        if (timed) prof_close(c, s, pe);
        HIPCHK(e);
    }
    return 0;
}

// the host threads of the pipeline (option host_threads, default 16: two thirds on the input side); the calling thread and the drain
// thread each count as one worker of their pool.  Stream pushes stage through the same pools.
void ensure_pools(b2f_ctx *c)
{
    const int nthreads = std::max(2, c->host_threads > 0 ? c->host_threads : (int)std::min(16u, std::thread::hardware_concurrency()));
    const int w_out = std::max(0, nthreads / 3 - 1), w_in = std::max(0, nthreads - nthreads / 3 - 1);
    if (!c->pool_in || c->pool_in->workers() != w_in) c->pool_in.reset(new CopyPool(w_in));
    if (!c->pool_out || c->pool_out->workers() != w_out) c->pool_out.reset(new CopyPool(w_out));
}

// check_request, then what both paths check of the context
int check_context(b2f_ctx *c, const FlowRequest &r)
{
    CHK(check_request(r));
    if (!c) return fail(std::string(r.who) + ": null context");
    if (r.seq && !c->g.shipped())
        return fail(std::string(r.who) + ": sequences run on the shipped graph only (this context was made with b2f_init_ex options)");
    if (r.o.want_past() && !c->past_flow)
        return fail(std::string(r.who) + ": this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only)");
    return 0;
}

// ---- streams ------------------------------------------------------------------------------------------------------------------
// push k (k0 = k - 1 pushes before it) writes ring slot k0 % 3 and reads the slots of the two pushes before it
StreamPass stream_pass(const b2f_stream *st)
{
    const int k0 = (int)(st->pushed % 3), s_ref = (k0 + 2) % 3, s_past = (k0 + 1) % 3;
    StreamPass sp;
    sp.ring = st->dev;
    sp.slot = k0;
    sp.ready = st->pushed >= 2;
    for (int l = 3; l <= 7; ++l) {
        sp.pyr[l] = st->lvl[k0][l];
        sp.fut[l] = st->lvl[k0][l];
        sp.ref[l] = st->lvl[s_ref][l];
        sp.past[l] = st->lvl[s_past][l];
    }
    sp.frame_past = st->frame[s_past];
    sp.frame_kind = st->frame_kind;
    if (st->flags & B2F_STREAM_WARP) {   // the caller's frames: the raw ring, or at a /64 size the frame slots themselves
        char *const *raw = st->raw[0] ? st->raw : st->frame;
        sp.raw_past = raw[s_past]; sp.raw_ref = raw[s_ref]; sp.raw_fut = raw[k0];
        sp.raw_kind = st->in_kind;
    }
    return sp;
}

// the slot of the raw ring a push writes (nullptr: the stream keeps none, or its frame slots serve)
char *raw_slot(const b2f_stream *st) { return st->raw[st->pushed % 3]; }

// what both push paths check before any HIP work: the request (check_request), the stream and its context
int check_push(const FlowRequest &r)
{
    const b2f_stream *st = r.stream;
    if (!st) return fail(std::string(r.who) + ": null stream");
    CHK(check_request(r));
    if (st->broken)
        return fail(std::string(r.who) + ": the stream is broken (a HIP call failed inside an earlier push): call b2f_stream_reset");
    if (!st->ctx->g.shipped())
        return fail(std::string(r.who) + ": streams run on the shipped graph only (this context was made with b2f_init_ex options)");
    if (r.o.want_past() && !st->ctx->past_flow)   // b2f_set_weights may have turned the context Hard since the stream was opened
        return fail(std::string(r.who) + ": this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only)");
    return 0;
}

// the device buffers of a push between its input and its outputs, and what the forward pass reads
struct PushPlan {
    Geometry g;
    StreamPass sp;
    NetBuffers net;
    const float *occ_net;   // skip_occs[3] at the network size
};

// want_prob: the push needs skip_occs[3] (occ_prob asked for, or a photometric record that is weighted with it); want_past: it runs the
// past-flow decoder chain into d_past
PushPlan push_plan(const b2f_stream *st, bool want_prob, bool want_past)
{
    PushPlan p;
    p.g = geometry(st->ctx, st->H0, st->W0);
    p.sp = stream_pass(st);
    p.net = {st->d_tmp, (float *)st->frame[p.sp.slot], st->d_flow, (want_prob && p.g.C3 == 3) ? st->d_occ : nullptr, st->d_est3};
    p.net.past = want_past ? st->d_past : nullptr;
    p.occ_net = p.g.C3 == 3 ? st->d_occ : st->d_est3;
    return p;
}

int push_host_work(b2f_stream *st, const FlowRequest &r, int k_in, const int *k_out)
{
    b2f_ctx *c = st->ctx;
    const FlowOutputs &o = r.o;
    HIPCHK(hipSetDevice(c->device));
    if (c->debug_fail_next) {   // tests (option debug_fail_next): one forced failure inside a push
        c->debug_fail_next = 0;
        return fail(std::string(r.who) + ": forced failure (option debug_fail_next)");
    }
    const ReqBatch req_guard(c, r);
    // the photometric record is weighted with occ_prob on the device whether or not the caller downloads it
    const bool want_prob = o.occ_prob != nullptr, need_prob = want_prob || o.photo != nullptr, want_rgb = o.rgb != nullptr;
    const bool want_past = o.want_past();
    const PushPlan P = push_plan(st, need_prob, want_past);
    const Geometry &g = P.g;
    const bool same = g.same, bytes_in = st->in_kind == B2F_IN_U8;
    const int n = st->cams;
    const size_t hw0 = g.hw0, in_bytes = (size_t)n * 3 * hw0 * (bytes_in ? 1 : 4);
    const size_t n_flow = (size_t)n * 2 * hw0 * 4, n_mask = (size_t)n * hw0, n_rgb = (size_t)n * 3 * hw0, n_max = (size_t)n * sizeof(double);
    // the outputs of the stream's flags (0 bytes without the flag: a plain stream stages what it always did)
    const size_t n_warp = (st->flags & B2F_STREAM_WARP) ? 2 * in_bytes : 0,
                 n_photo = (st->flags & B2F_STREAM_WARP) ? (size_t)n * B2F_PHOTO_WORDS * sizeof(unsigned long long) : 0,
                 n_past = (st->flags & B2F_STREAM_PAST) ? n_flow : 0;
    // staging of pageable buffers: [frames | flow | occ_prob | fwd | bwd | rgb | max | warped | photo | past_flow], allocated with the
    // first pageable push
    constexpr int kOuts = 9;
    size_t offs[kOuts + 2] = {0};
    const size_t parts[kOuts + 1] = {in_bytes, n_flow, n_flow, n_mask, n_mask, n_rgb, n_max, n_warp, n_photo, n_past};
    for (int i = 0; i <= kOuts; ++i) offs[i + 1] = offs[i] + align256(parts[i]);
    bool pageable = k_in != 1;
    for (int i = 0; i < kOuts; ++i) pageable = pageable || k_out[i] != 1;
    if (pageable && !st->pin) {
        HIPCHK(hipHostMalloc(&st->pin, offs[kOuts + 1], hipHostMallocDefault));
        st->pin_bytes = offs[kOuts + 1];
    }
    if (pageable) ensure_pools(c);   // the context's host threads do the staging copies
    hipStream_t s = c->stream;
    // ---- one upload of the cams frames: into their frame slot at a /64 size, else into the buffers image.scale reads -- or, on a
    // stream that keeps the caller's frames for the warp, into the push's slot of the raw ring, which then stands in for them
    char *const raw = raw_slot(st);
    unsigned char *const up_u8 = raw ? (unsigned char *)raw : st->d_u8;
    const float *const up_f32 = (raw && !bytes_in) ? (const float *)raw : st->d_up;   // what image.scale reads
    void *dst = same ? (void *)st->frame[P.sp.slot] : bytes_in ? (void *)up_u8 : (void *)up_f32;
    const void *src = r.im1;
    if (k_in != 1) {
        c->pool_in->run({{st->pin, r.im1, in_bytes}});
        src = st->pin;
    }
    HIPCHK(hipMemcpyAsync(dst, src, in_bytes, hipMemcpyHostToDevice, s));
    if (!same && bytes_in) HIPCHK(launch_unpack_u8(up_u8, (size_t)n * 3 * hw0, st->d_up, s));
    FlowOutputs d{nullptr, same ? nullptr : st->d_flow32, (need_prob && !same) ? st->d_prob : nullptr, o.fwd_occ ? st->d_fo : nullptr,
                  o.bwd_occ ? st->d_bo : nullptr, want_rgb ? st->d_rgb : nullptr, want_rgb ? st->d_max : nullptr, o.max_norm, o.rgb_layout};
    d.flow_scale = o.flow_scale; d.warping = o.warping;
    d.warped = o.warped ? st->d_warp : nullptr; d.warped_kind = o.warped_kind;
    d.photo = o.photo ? st->d_photo : nullptr;
    d.past32 = (want_past && !same) ? st->d_past32 : nullptr; d.own_past = o.own_past;
    CHK(run_kernels(c, r, g, same ? (const void *)st->frame[P.sp.slot] : up_f32, same ? st->in_kind : B2F_IN_UNIT, (long)n * 3, n, P.net, d,
                    c->host_graph != 0, s, &P.sp));
    // ---- download what was asked for: page-locked buffers in place, pageable ones through the staging block
    struct Down { void *host; const void *dev; size_t bytes; int kind; size_t off; };
    const Down downs[kOuts] = {{o.flow32, st->d_flow32, n_flow, k_out[0], offs[1]}, {o.occ_prob, same ? (const void *)P.occ_net : st->d_prob, n_flow, k_out[3], offs[2]},
                               {o.fwd_occ, st->d_fo, n_mask, k_out[1], offs[3]}, {o.bwd_occ, st->d_bo, n_mask, k_out[2], offs[4]},
                               {o.rgb, st->d_rgb, n_rgb, k_out[4], offs[5]}, {o.rgb_max, st->d_max, n_max, k_out[5], offs[6]},
                               {o.warped, st->d_warp, n_warp, k_out[6], offs[7]}, {o.photo, st->d_photo, n_photo, k_out[7], offs[8]},
                               {o.past32, st->d_past32, n_past, k_out[8], offs[9]}};
    std::vector<CopyJob> jobs;
    for (const Down &d : downs) {
        if (!d.host || !P.sp.ready) continue;
        HIPCHK(hipMemcpyAsync(d.kind == 1 ? d.host : (void *)(st->pin + d.off), d.dev, d.bytes, hipMemcpyDeviceToHost, s));
        if (d.kind != 1) jobs.push_back({d.host, st->pin + d.off, d.bytes});
    }
    HIPCHK(hipStreamSynchronize(s));
    if (!jobs.empty()) c->pool_out->run(jobs);
    return 0;
}

int push_device_work(b2f_stream *st, const FlowRequest &r, hipStream_t s)
{
    b2f_ctx *c = st->ctx;
    HIPCHK(hipSetDevice(c->device));
    const ReqBatch req_guard(c, r);
    FlowOutputs o = r.o;
    const PushPlan P = push_plan(st, o.occ_prob != nullptr || o.photo != nullptr, o.want_past());
    const Geometry &g = P.g;
    const bool bytes_in = st->in_kind == B2F_IN_U8;
    const int n = st->cams;
    const size_t samples = (size_t)n * 3 * g.hw0;
    const void *x = r.im1;   // a rescaled float stream: image.scale reads the caller's frames themselves
    if (g.same) {
        // the frames must outlive the call (est[3] of a Hard model warps them two pushes later): into their frame slot
        HIPCHK(hipMemcpyAsync(st->frame[P.sp.slot], r.im1, samples * (bytes_in ? 1 : 4), hipMemcpyDeviceToDevice, s));
        x = st->frame[P.sp.slot];
    } else {
        // a stream that keeps the caller's frames for the warp: into the push's slot of the raw ring
        if (char *raw = raw_slot(st)) HIPCHK(hipMemcpyAsync(raw, r.im1, samples * (bytes_in ? 1 : 4), hipMemcpyDeviceToDevice, s));
        if (bytes_in) {
            HIPCHK(launch_unpack_u8((const unsigned char *)r.im1, samples, st->d_up, s));
            x = st->d_up;
        }
    }
    if (!g.same) {   // what the warp of a rescaled flow reads at H0 x W0 and the caller left out: the stream's own buffers
        if (o.warping && !o.flow32) o.flow32 = st->d_flow32;
        if (o.photo && !o.occ_prob) o.occ_prob = st->d_prob;
        if (o.own_past && !o.past32) o.past32 = st->d_past32;
    }
    return run_kernels(c, r, g, x, g.same ? st->in_kind : B2F_IN_UNIT, (long)n * 3, n, P.net, o, c->use_graph != 0, s, &P.sp);
}

}  // namespace

int b2f::check_request(const FlowRequest &r)
{
    const std::string w(r.who);
    if (r.in_kind == B2F_IN_NORMALIZED)
        return fail(w + ": in_kind B2F_IN_NORMALIZED is refused: computeFlow normalizes its frames itself (B2F_IN_UNIT or B2F_IN_U8)");
    if (r.in_kind != B2F_IN_UNIT && r.in_kind != B2F_IN_U8) return fail(w + ": in_kind must be B2F_IN_UNIT or B2F_IN_U8");
    if (r.seq && r.n <= 0) return fail(w + ": a sequence needs T >= 3 frames (one triplet)");
    if (r.n <= 0 || r.H0 <= 0 || r.W0 <= 0) return fail(w + ": bad shape");
    if (r.H0 < 64 || r.W0 < 64) return fail(w + ": image smaller than 64 pixels");
    const FlowOutputs &o = r.o;
    // an rgb request (f32 path) needs its pictures and may leave the flow out
    // a score request (f32 path too) needs its records and the ground-truth flow
    if (!r.im1 || (!r.seq && !r.stream && (!r.im2 || !r.im3)) ||
        (!o.f32() ? !o.fwd_occ || !o.bwd_occ : o.pictures ? !o.rgb : o.scoring ? !o.scores || !o.gt_flow : o.warping ? false : !o.flow32))
        return fail(w + ": null argument");
    // the past flow is an output of the float32 batch and sequence entries of a Soft model (the model is check_context's to refuse)
    // ... and of a stream that was opened for it
    if (o.want_past()) {
        if (r.stream && !(r.stream->flags & B2F_STREAM_PAST))
            return fail(w + ": this stream was opened without B2F_STREAM_PAST (b2f_stream_open_ex): it does not return the past flow");
        if (!o.f32()) return fail(w + ": the past flow is an output of the float32 entries");
        if (o.own_past && !o.warping) return fail(w + ": only a warp request can use the model's own past flow");
    }
    // a warp request (f32 path as well) needs the warped frames or the photometric records; a stream keeps the frames it samples
    // only when it was opened for it
    if (o.warping) {
        if (r.stream && !(r.stream->flags & B2F_STREAM_WARP))
            return fail(w + ": this stream was opened without B2F_STREAM_WARP (b2f_stream_open_ex): it keeps no frames to warp");
        if (!o.f32()) return fail(w + ": warped frames are an output of the float32 batch and sequence entries");
        if (!(o.flow_scale > 0.0) || !std::isfinite(o.flow_scale)) return fail(w + ": flow_scale must be finite and > 0");
        if ((long long)r.H0 * r.W0 >= (1ll << 28)) return fail(w + ": images of 2^28 pixels or more are refused (the Q30 sums could overflow)");
        if (!o.warped && !o.photo) return fail(w + ": at least one of warped and photo is required");
    }
    if (o.scoring) {
        if (!o.f32() || r.stream) return fail(w + ": scores are an output of the float32 batch and sequence entries");
        if (!(o.flow_scale > 0.0) || !std::isfinite(o.flow_scale)) return fail(w + ": flow_scale must be finite and > 0");
        if ((long long)r.H0 * r.W0 >= (1ll << 28)) return fail(w + ": images of 2^28 pixels or more are refused (the Q20 sums could overflow)");
    }
    if (o.pictures && (!o.f32() || (o.rgb_layout != B2F_RGB_PLANAR && o.rgb_layout != B2F_RGB_PACKED)))
        return fail(w + ": bad layout (B2F_RGB_PLANAR or B2F_RGB_PACKED)");
    return 0;
}

// ---- host buffers: a double-buffered upload / compute / download pipeline --------------------------------------------------------
// The n triplets are cut into sub-batches (up to B2F_HOST_SUBBATCH_PIXELS input pixels each, default 16 Mpx = eight
// full-HD triplets) that flow through two buffer sets on three streams: uploads on s_in, ColorNormalize /
// image.scale / the network / the nearest rescale + thresholds on the context's stream, downloads on s_out.
// A buffer set's input half is reused as soon as the kernels that read it are done and its output half as soon
// as its download has been handed over, so in steady state all three streams are busy.
// The link is the bound of this entry point (one MI355X box: 56 GB/s in either direction, but only 55 GB/s for
// both together), so both directions carry as few bytes as exactness allows: inputs that are k / 255 go up as
// bytes (pack_u8_piece), the flow comes down as the network's fp32 values and becomes `double * sc` on the host
// (back2future.lua:80-84), exactly the reference's arithmetic.  Host threads (option host_threads, default 16, two
// thirds on the input side; the output side is driven by a second control thread) do the packing / staging and
// the f32 -> f64 conversion; page-locked caller buffers are DMA'd in place where no conversion is involved.
// Sequence mode (seq, b2f_compute_flow_sequence*): im1 holds n + 2 frames (T x 3 x H0 x W0) and triplet b is frames
// (b, b + 1, b + 2).  A sub-batch of nb triplets uploads its nb + 2 frames once -- the two it shares with the next
// sub-batch go up (and through the pyramid) again there -- and runs the sequence forward; everything else is the
// triplet pipeline with "frame" in place of "triplet" as the unit of upload, 8-bit detection and the sub-batch budget.
// Outputs (FlowOutputs): the f64 path widens the flow on the host threads; the f32 path (b2f_*_f32) has the device write
// every output in its final form (outputs_f32_kernel), so the drain step only copies -- or nothing at all: page-locked
// flow / occ_prob / mask buffers are DMA'd in place -- and a NULL occ_prob or mask is neither written nor downloaded.  The pictures
// and maxima of an rgb request (b2f_*_rgb) travel like occ_prob: slot buffers, DMA in place or staging + drain copy; its flow stays
// on the device unless asked for.  A score request (b2f_*_score) uploads the ground truth of every sub-batch's outputs with its frames
// (page-locked buffers in place, pageable ones through the slot's staging block) and downloads the 176-byte records.  A warp
// request (b2f_*_warp) downloads the warped neighbours and the 112-byte photometric records like the pictures; whatever else it
// leaves out stays on the device.
int b2f::compute_flow_host(b2f_ctx *c, const FlowRequest &r)
{
    CHK(check_context(c, r));
    const std::string w(r.who);
    HIPCHK(hipSetDevice(c->device));
    const FlowOutputs &o = r.o;
    const int n = r.n;
    const bool seq = r.seq, f32 = o.f32(), bytes_in = r.in_kind == B2F_IN_U8;
    const Geometry g = geometry(c, r.H0, r.W0);
    const size_t hw0 = g.hw0;
    const bool same = g.same;
    const size_t esz = bytes_in ? 1 : 4;   // bytes per input sample in the caller's buffers
    const int gu = seq ? 2 : 0;            // frames of a sequence beyond its triplets
    const int k_in[3] = {mem_kind(r.im1, (size_t)(n + gu) * 3 * hw0 * esz), seq ? 1 : mem_kind(r.im2, (size_t)n * 3 * hw0 * esz),
                         seq ? 1 : mem_kind(r.im3, (size_t)n * 3 * hw0 * esz)};
    double *flow = o.flow64;
    unsigned char *fwd_occ = o.fwd_occ, *bwd_occ = o.bwd_occ;
    // unrequested outputs (f32 path) count as page-locked: nothing is staged for them
    auto out_kind = [&](const void *p, size_t bytes) { return p ? mem_kind(p, bytes) : 1; };
    const int k_out[6] = {f32 ? out_kind(o.flow32, (size_t)n * 2 * hw0 * 4) : mem_kind(flow, (size_t)n * 2 * hw0 * 8), out_kind(fwd_occ, (size_t)n * hw0),
                          out_kind(bwd_occ, (size_t)n * hw0), out_kind(o.occ_prob, (size_t)n * 2 * hw0 * 4), out_kind(o.rgb, (size_t)n * 3 * hw0),
                          out_kind(o.rgb_max, (size_t)n * sizeof(double))};
    // a score request: the ground truth (inputs; absent planes count as page-locked) and the records
    const int k_gt[4] = {out_kind(o.gt_flow, (size_t)n * 2 * hw0 * 4), out_kind(o.valid, (size_t)n * hw0), out_kind(o.gt_occ, (size_t)n * hw0),
                         out_kind(o.scores, (size_t)n * B2F_SCORE_WORDS * sizeof(unsigned long long))};
    // a warp request: the warped neighbours in the frames' element type and the records
    const size_t warp_esz = o.warped ? (o.warped_kind == B2F_IN_U8 ? 1 : 4) : 0;
    const int k_wp[2] = {out_kind(o.warped, (size_t)n * 6 * hw0 * warp_esz), out_kind(o.photo, (size_t)n * B2F_PHOTO_WORDS * sizeof(unsigned long long))};
    const bool want_past = o.want_past();
    const int k_past = out_kind(o.past32, (size_t)n * 2 * hw0 * 4);
    for (int i = 0; i < 6; ++i)
        if ((i < 3 && k_in[i] < 0) || k_out[i] < 0 || (i < 4 && k_gt[i] < 0) || (i < 2 && k_wp[i] < 0) || k_past < 0)
            return fail(w + ": device memory passed to a host-buffer entry point (use b2f_compute_flow_device / "
                            "b2f_compute_flow_sequence_device)");
    if (c->debug_fail_next) {   // tests (option debug_fail_next): one forced failure, e.g. on one replica of a b2f_multi
        c->debug_fail_next = 0;
        return fail(w + ": forced failure (option debug_fail_next)");
    }
    const ReqBatch req_guard(c, r);
    const bool use_u8 = bytes_in || c->host_u8 != 0;
    int SB = 0;
    const std::vector<std::pair<int, int>> subs = plan_subbatches(c, n, seq, hw0, c->host_ramp != 0, &SB);
    const int nsub = (int)subs.size();

    if (!c->s_in) HIPCHK(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
    if (!c->s_out) HIPCHK(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
    const bool pinned_in = k_in[0] == 1 && k_in[1] == 1 && k_in[2] == 1;
    const bool stage_in = !pinned_in && !bytes_in;   // float staging buffer (byte inputs stage through h_u8)
    const bool stage_masks = !(k_out[1] == 1 && k_out[2] == 1);
    const bool want_prob = f32 && o.occ_prob;
    const bool want_score = o.scores != nullptr;
    // the occlusion scores read occ_prob on the device whether or not the caller downloads it
    // ... and so do the photometric records, for their weights
    const bool want_photo = o.photo != nullptr;
    const bool need_prob = want_prob || (want_score && o.gt_occ) || want_photo;
    // f32 path: occ_prob is skip_occs[3] -- est[3] of a Soft model (d_est3), an extra forward output of a Hard one (d_occ)
    const bool want_rgb = o.rgb != nullptr;
    SlotNeeds q{same, stage_in, stage_masks, use_u8, need_prob && g.C3 == 3, need_prob && !same, !f32 || k_out[0] != 1, want_prob && k_out[3] != 1,
                want_rgb, want_rgb && k_out[4] != 1, want_rgb && k_out[5] != 1,
                want_score, want_score && o.valid, want_score && o.gt_occ, want_score && k_gt[0] != 1, want_score && o.valid && k_gt[1] != 1,
                want_score && o.gt_occ && k_gt[2] != 1, want_score && k_gt[3] != 1,
                warp_esz, want_photo, o.warped && k_wp[0] != 1, want_photo && k_wp[1] != 1,
                want_past, o.past32 && k_past != 1};
    // (a sequence sub-batch's nb + 2 frames are 3 nb + 6 <= 9 nb planes: the triplet layout of the slot holds them)
    for (int k = 0; k < std::min(nsub, 2); ++k)
        CHK(ensure_slot(c, c->slot[k], SB, hw0, g.hw, g.H0, g.fw, g.C3, q));
    ensure_pools(c);

    const char *ims[3] = {(const char *)r.im1, (const char *)r.im2, (const char *)r.im3};
    // upload units: a triplet (3 frames, one from each of im1..im3) or, in sequence mode, one frame; frame f of unit u of
    // a sub-batch starting at triplet b0 comes from src(b0 + u, f) and lands at plane (u * fpu + f) * 3 of the slot
    const int fpu = seq ? 1 : 3;
    auto src = [&](size_t u, int f) { return ims[seq ? 0 : f] + u * 3 * hw0 * esz; };
    // ---- output side: a second control thread hands finished downloads to the caller ----
    std::mutex mu;
    std::condition_variable cv;
    int submitted = 0, drained = 0;   // sub-batches whose downloads are enqueued / handed over (guarded by mu)
    bool abort = false;
    std::string drain_err;
    auto drain_loop = [&]() {
        (void)hipSetDevice(c->device);
        for (int k = 0; k < nsub; ++k) {
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return submitted > k || abort; });
                if (abort) return;
            }
            HostSlot &hs = c->slot[k & 1];
            const hipError_t e = hipEventSynchronize(hs.ev_out);
            if (e == hipSuccess) {
                const size_t b0 = subs[k].first, nb = (size_t)subs[k].second;
                std::vector<CopyJob> jobs;
                if (!f32) {
                    // flow_est[1] * sc_w, flow_est[2] * sc_h on the :double() copy of est[1] (:80-84)
                    for (size_t t = 0; t < nb; ++t)
                        for (int ch = 0; ch < 2; ++ch)
                            jobs.push_back({flow + ((b0 + t) * 2 + ch) * hw0, hs.h_flow32 + (t * 2 + ch) * hw0, hw0 * 4, JOB_F32_TO_F64,
                                            ch == 0 ? g.sc_w : g.sc_h, nullptr});
                } else {
                    if (q.stage_flow) jobs.push_back({o.flow32 + b0 * 2 * hw0, hs.h_flow32, nb * 2 * hw0 * 4});
                    if (q.stage_prob) jobs.push_back({o.occ_prob + b0 * 2 * hw0, hs.h_prob, nb * 2 * hw0 * 4});
                    if (q.stage_rgb) jobs.push_back({o.rgb + b0 * 3 * hw0, hs.h_rgb, nb * 3 * hw0});
                    if (q.stage_max) jobs.push_back({o.rgb_max + b0, hs.h_max, nb * sizeof(double)});
                    if (q.stage_score) jobs.push_back({o.scores + b0 * B2F_SCORE_WORDS, hs.h_score, nb * B2F_SCORE_WORDS * sizeof(unsigned long long)});
                    if (q.stage_warp) jobs.push_back({(char *)o.warped + b0 * 6 * hw0 * warp_esz, hs.h_warp, nb * 6 * hw0 * warp_esz});
                    if (q.stage_photo) jobs.push_back({o.photo + b0 * B2F_PHOTO_WORDS, hs.h_photo, nb * B2F_PHOTO_WORDS * sizeof(unsigned long long)});
                    if (q.stage_past) jobs.push_back({o.past32 + b0 * 2 * hw0, hs.h_past, nb * 2 * hw0 * 4});
                }
                if (stage_masks) {
                    if (fwd_occ) jobs.push_back({fwd_occ + b0 * hw0, hs.h_fo, nb * hw0});
                    if (bwd_occ) jobs.push_back({bwd_occ + b0 * hw0, hs.h_bo, nb * hw0});
                }
                c->pool_out->run(jobs);
            }
            std::lock_guard<std::mutex> l(mu);
            if (e != hipSuccess) {
                drain_err = std::string("download failed: ") + hipGetErrorString(e);
                abort = true;
            }
            drained = k + 1;
            cv.notify_all();
            if (abort) return;
        }
    };
    std::thread drainer(drain_loop);
    struct Joiner {   // an exception on the way out (std::bad_alloc ...) must not leave the thread running
        std::thread &t; std::mutex &mu; std::condition_variable &cv; bool &abort;
        ~Joiner()
        {
            if (!t.joinable()) return;
            { std::lock_guard<std::mutex> l(mu); abort = true; }
            cv.notify_all();
            t.join();
        }
    } joiner{drainer, mu, cv, abort};

    bool try_u8 = use_u8;             // off for the rest of the call after the first triplet that is not 8-bit data
    std::atomic<int> inexact{0};
    auto submit = [&](int k) -> int {
        HostSlot &hs = c->slot[k & 1];
        const size_t b0 = subs[k].first;
        const int nb = subs[k].second;
        // ---- upload: torch.cat({im1, im2, im3}, 1) (back2future.lua:48) = [triplet][frame][3][H0][W0] on the device.
        // The set's staging buffers are free once upload k - 2 has left them, its device buffers once the kernels
        // of k - 2 are done (both events still hold the records of k - 2 here).
        if (k >= 2) HIPCHK(hipEventSynchronize(hs.ev_in));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(c->s_in, hs.ev_comp, 0));
        const int nu = nb + gu;
        std::vector<int> as_u8(nu, 0);
        for (int t = 0; t < nu; ++t) {
            const size_t u0 = (size_t)t * fpu * 3 * hw0;   // first sample of unit t in the slot
            float *dst = hs.d_up + u0;
            if (bytes_in) {   // the caller's samples are the bytes: value = k / 255
                unsigned char *du = hs.d_u8 + u0;
                if (pinned_in) {
                    for (int f = 0; f < fpu; ++f)
                        HIPCHK(hipMemcpyAsync(du + (size_t)f * 3 * hw0, src(b0 + t, f), 3 * hw0, hipMemcpyHostToDevice, c->s_in));
                } else {
                    unsigned char *st = hs.h_u8 + u0;
                    for (int f = 0; f < fpu; ++f) {   // frame by frame: the DMA of one frame runs under the staging copy of the next
                        c->pool_in->run({{st + (size_t)f * 3 * hw0, src(b0 + t, f), 3 * hw0}});
                        HIPCHK(hipMemcpyAsync(du + (size_t)f * 3 * hw0, st + (size_t)f * 3 * hw0, 3 * hw0, hipMemcpyHostToDevice, c->s_in));
                    }
                }
                as_u8[t] = 1;
                continue;
            }
            if (try_u8) {
                unsigned char *st = hs.h_u8 + u0;
                // frame by frame: the DMA of a packed frame runs under the packing of the next.  A frame that turns
                // out not to be 8-bit data sends the whole unit down the float path (its earlier frames are
                // uploaded twice; d_up is what the kernels read for it).
                for (int f = 0; f < fpu && !inexact.load(); ++f) {
                    c->pool_in->run({{st + (size_t)f * 3 * hw0, src(b0 + t, f), 3 * hw0 * 4, JOB_PACK_U8, 1.0, &inexact}});
                    if (!inexact.load())
                        HIPCHK(hipMemcpyAsync(hs.d_u8 + u0 + (size_t)f * 3 * hw0, st + (size_t)f * 3 * hw0, 3 * hw0,
                                              hipMemcpyHostToDevice, c->s_in));
                }
                if (!inexact.load()) {
                    as_u8[t] = 1;
                    continue;
                }
                try_u8 = false;
            }
            if (stage_in) {
                float *st = hs.h_in + u0;
                for (int f = 0; f < fpu; ++f) {
                    c->pool_in->run({{st + (size_t)f * 3 * hw0, src(b0 + t, f), 3 * hw0 * 4}});
                    HIPCHK(hipMemcpyAsync(dst + (size_t)f * 3 * hw0, st + (size_t)f * 3 * hw0, 3 * hw0 * 4, hipMemcpyHostToDevice, c->s_in));
                }
            } else {
                for (int f = 0; f < fpu; ++f)
                    HIPCHK(hipMemcpyAsync(dst + (size_t)f * 3 * hw0, src(b0 + t, f), 3 * hw0 * 4, hipMemcpyHostToDevice, c->s_in));
            }
        }
        if (want_score) {   // the ground truth of the sub-batch's nb outputs goes up with its frames
            struct Up { void *dev; void *pin; const void *host; size_t bytes; bool stage; };
            const Up ups[3] = {{hs.d_gt, hs.h_gt, o.gt_flow + b0 * 2 * hw0, (size_t)nb * 2 * hw0 * 4, q.stage_gt},
                               {hs.d_valid, hs.h_valid, o.valid ? o.valid + b0 * hw0 : nullptr, (size_t)nb * hw0, q.stage_valid},
                               {hs.d_gtocc, hs.h_gtocc, o.gt_occ ? o.gt_occ + b0 * hw0 : nullptr, (size_t)nb * hw0, q.stage_gtocc}};
            for (const Up &u : ups) {
                if (!u.host) continue;
                if (u.stage) c->pool_in->run({{u.pin, u.host, u.bytes}});
                HIPCHK(hipMemcpyAsync(u.dev, u.stage ? u.pin : u.host, u.bytes, hipMemcpyHostToDevice, c->s_in));
            }
        }
        HIPCHK(hipEventRecord(hs.ev_in, c->s_in));
        // ---- kernels: after the upload, and after download k - 2 has read this set's output buffers
        HIPCHK(hipStreamWaitEvent(c->stream, hs.ev_in, 0));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(c->stream, hs.ev_out, 0));
        // a /64 sequence that crossed the link as bytes only: the sequence forward reads the bytes themselves
        const bool direct_u8 = seq && same && std::all_of(as_u8.begin(), as_u8.end(), [](int v) { return v != 0; });
        for (int t = 0; t < nu && !direct_u8; ++t)
            if (as_u8[t]) HIPCHK(launch_unpack_u8(hs.d_u8 + (size_t)t * fpu * 3 * hw0, (size_t)fpu * 3 * hw0, hs.d_up + (size_t)t * fpu * 3 * hw0, c->stream));
        // without a rescale the flow and occ_prob planes are the network's, downloaded as they are
        const float *occ_net = g.C3 == 3 ? hs.d_occ : hs.d_est3;
        CHK(run_kernels(c, r, g, direct_u8 ? (const void *)hs.d_u8 : hs.d_up, direct_u8 ? B2F_IN_U8 : B2F_IN_UNIT, (long)nu * fpu * 3, nb,
                        {hs.d_tmp, hs.d_in, hs.d_flow, hs.d_occ, hs.d_est3, hs.d_past},
                        {nullptr, same ? nullptr : hs.d_flow32, q.prob ? hs.d_prob : nullptr, fwd_occ ? hs.d_fo : nullptr, bwd_occ ? hs.d_bo : nullptr,
                         hs.d_rgb, hs.d_max, o.max_norm, o.rgb_layout, o.pictures,
                         hs.d_score, hs.d_gt, hs.d_valid, hs.d_gtocc, o.flow_scale, o.scoring,
                         hs.d_warp, o.warped_kind, hs.d_photo, o.warping,
                         (q.past && !same) ? hs.d_past32 : nullptr, o.own_past},
                        c->host_graph != 0, c->stream));
        HIPCHK(hipEventRecord(hs.ev_comp, c->stream));
        // ---- download: the set's pinned output buffers must have been handed over (k - 2 drained)
        if (k >= 2) {
            std::unique_lock<std::mutex> l(mu);
            cv.wait(l, [&] { return drained >= k - 1 || abort; });
            if (abort) return fail(drain_err);
        }
        HIPCHK(hipStreamWaitEvent(c->s_out, hs.ev_comp, 0));
        if (!f32 || o.flow32)   // an rgb request may leave the flow on the device
            HIPCHK(hipMemcpyAsync(q.stage_flow ? hs.h_flow32 : o.flow32 + b0 * 2 * hw0, hs.d_flow32, (size_t)nb * 2 * hw0 * 4, hipMemcpyDeviceToHost,
                                  c->s_out));
        if (want_rgb)
            HIPCHK(hipMemcpyAsync(q.stage_rgb ? hs.h_rgb : o.rgb + b0 * 3 * hw0, hs.d_rgb, (size_t)nb * 3 * hw0, hipMemcpyDeviceToHost, c->s_out));
        if (o.rgb_max)
            HIPCHK(hipMemcpyAsync(q.stage_max ? hs.h_max : o.rgb_max + b0, hs.d_max, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->s_out));
        if (want_score)
            HIPCHK(hipMemcpyAsync(q.stage_score ? hs.h_score : o.scores + b0 * B2F_SCORE_WORDS, hs.d_score,
                                  (size_t)nb * B2F_SCORE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_out));
        if (o.warped)
            HIPCHK(hipMemcpyAsync(q.stage_warp ? hs.h_warp : (void *)((char *)o.warped + b0 * 6 * hw0 * warp_esz), hs.d_warp,
                                  (size_t)nb * 6 * hw0 * warp_esz, hipMemcpyDeviceToHost, c->s_out));
        if (want_photo)
            HIPCHK(hipMemcpyAsync(q.stage_photo ? hs.h_photo : o.photo + b0 * B2F_PHOTO_WORDS, hs.d_photo,
                                  (size_t)nb * B2F_PHOTO_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_out));
        if (o.past32)
            HIPCHK(hipMemcpyAsync(q.stage_past ? hs.h_past : o.past32 + b0 * 2 * hw0, hs.d_past32, (size_t)nb * 2 * hw0 * 4, hipMemcpyDeviceToHost,
                                  c->s_out));
        if (want_prob)
            HIPCHK(hipMemcpyAsync(q.stage_prob ? hs.h_prob : o.occ_prob + b0 * 2 * hw0, same ? occ_net : hs.d_prob, (size_t)nb * 2 * hw0 * 4,
                                  hipMemcpyDeviceToHost, c->s_out));
        if (fwd_occ)
            HIPCHK(hipMemcpyAsync(stage_masks ? hs.h_fo : fwd_occ + b0 * hw0, hs.d_fo, (size_t)nb * hw0, hipMemcpyDeviceToHost, c->s_out));
        if (bwd_occ)
            HIPCHK(hipMemcpyAsync(stage_masks ? hs.h_bo : bwd_occ + b0 * hw0, hs.d_bo, (size_t)nb * hw0, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(hipEventRecord(hs.ev_out, c->s_out));
        {
            std::lock_guard<std::mutex> l(mu);
            submitted = k + 1;
        }
        cv.notify_all();
        return 0;
    };
    int rc = 0;
    for (int k = 0; k < nsub && !rc; ++k) rc = submit(k);
    std::string msg = rc ? api_error() : std::string();
    if (rc) {
        std::lock_guard<std::mutex> l(mu);
        abort = true;
    }
    cv.notify_all();
    drainer.join();
    if (!rc && abort) { rc = 1; msg = drain_err; }
    // nothing of this call may still be in flight when the caller gets its buffers back
    for (hipStream_t st : {c->s_in, c->stream, c->s_out}) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && !rc) { rc = 1; msg = w + ": " + hipGetErrorString(e); }
    }
    if (rc) {
        (void)hipGetLastError();
        return fail(msg);
    }
    return 0;
}

// ---- device buffers: the kernels half of the pipeline's submit() on caller buffers, no transfers --------------------------------
// Per sub-batch, on the caller's stream: gather the three frame sets into B x 9 x H0 x W0 (triplets) and unpack bytes, then
// run_kernels into the caller's buffers.  Sub-batches follow the host pipeline's budget (no ramp: there is no upload to overlap) and a
// sequence's overlap by two frames; the buffers in between are the context's (c->dwork).  Every choice -- input kind of the forward
// pass, unpacking, the kernel rule of the request's n -- is the host pipeline's, so the results are the f32 host entries' bit for bit.
int b2f::compute_flow_device(b2f_ctx *c, const FlowRequest &r, void *stream)
{
    CHK(check_context(c, r));
    const std::string w(r.who);
    const FlowOutputs &o = r.o;
    const uintptr_t al = (uintptr_t)r.im1 | (uintptr_t)r.im2 | (uintptr_t)r.im3 | (uintptr_t)o.flow32 | (uintptr_t)o.occ_prob |
                         (uintptr_t)o.fwd_occ | (uintptr_t)o.bwd_occ | (uintptr_t)o.past32;
    if (al & 15) return fail(w + ": device buffers must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    const int n = r.n;
    const bool seq = r.seq, bytes_in = r.in_kind == B2F_IN_U8;
    const Geometry g = geometry(c, r.H0, r.W0);
    const size_t hw0 = g.hw0, esz = bytes_in ? 1 : 4;
    {
        const size_t in_bytes = (size_t)(seq ? n + 2 : n) * 3 * hw0 * esz, hw0n = (size_t)n * hw0;
        const std::pair<const void *, size_t> bufs[8] = {{r.im1, in_bytes}, {r.im2, in_bytes}, {r.im3, in_bytes}, {o.flow32, hw0n * 8},
                                                         {o.occ_prob, hw0n * 8}, {o.fwd_occ, hw0n}, {o.bwd_occ, hw0n}, {o.past32, hw0n * 8}};
        for (const auto &pb : bufs)
            if (pb.first && mem_kind(pb.first, pb.second) >= 0)
                return fail(w + ": host memory passed to a device entry point (use b2f_compute_flow_batch_f32 / b2f_compute_flow_sequence_f32)");
    }
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const ReqBatch req_guard(c, r);
    int SB = 0;
    const std::vector<std::pair<int, int>> subs = plan_subbatches(c, n, seq, hw0, false, &SB);
    // workspace: bytes of the gathered triplets, their floats, image.scale's two passes, the network's outputs
    const bool unpack = bytes_in && !(seq && g.same);   // a /64 byte sequence is read as it is (the pipeline's direct_u8)
    const size_t planes = (size_t)(seq ? SB + 2 : SB) * (seq ? 3 : 9);
    const size_t n_u8 = (!seq && bytes_in) ? align256(planes * hw0) : 0, n_up = (!seq || unpack) ? align256(planes * hw0 * 4) : 0,
                 n_tmp = g.same ? 0 : align256(planes * g.H0 * g.fw * 4), n_in = g.same ? 0 : align256(planes * g.hw * 4),
                 n_flow = align256((size_t)SB * 2 * g.hw * 4), n_occ = (o.occ_prob && g.C3 == 3) ? n_flow : 0,
                 n_est3 = align256((size_t)SB * g.C3 * g.hw * 4), n_past = o.want_past() ? n_flow : 0;
    const size_t need = n_u8 + n_up + n_tmp + n_in + n_flow + n_occ + n_est3 + n_past;
    DevWork &dw = c->dwork;
    if (need > dw.bytes) {
        if (dw.dev) {
            HIPCHK(hipDeviceSynchronize());   // earlier calls may still read it, on any stream
            HIPCHK(hipFree(dw.dev));
            dw.dev = nullptr; dw.bytes = 0;
            drop_graphs(c);                   // graphs are keyed on its pointers
        }
        HIPCHK(hipMalloc(&dw.dev, need));
        dw.bytes = need;
    }
    char *d = dw.dev;
    unsigned char *d_u8 = (unsigned char *)d; d += n_u8;
    float *d_up = (float *)d; d += n_up;
    NetBuffers net;
    net.tmp = (float *)d; d += n_tmp;
    net.scaled = (float *)d; d += n_in;
    net.flow = (float *)d; d += n_flow;
    net.occ = n_occ ? (float *)d : nullptr; d += n_occ;
    net.est3 = (float *)d; d += n_est3;
    net.past = n_past ? (float *)d : nullptr;
    const char *ims[3] = {(const char *)r.im1, (const char *)r.im2, (const char *)r.im3};
    for (const auto &sb : subs) {
        const int b0 = sb.first, nb = sb.second;
        const size_t np = (size_t)(seq ? nb + 2 : nb) * (seq ? 3 : 9);   // input planes of this sub-batch
        const void *x = d_up;   // what the forward pass reads
        int kind = B2F_IN_UNIT;
        if (!seq) {   // torch.cat({im1, im2, im3}, 1) (back2future.lua:48): triplet t's frames f = 0..2 at planes (t * 3 + f) * 3
            char *gp = bytes_in ? (char *)d_u8 : (char *)d_up;
            for (int t = 0; t < nb; ++t)
                for (int f = 0; f < 3; ++f)
                    HIPCHK(hipMemcpyAsync(gp + ((size_t)t * 3 + f) * 3 * hw0 * esz, ims[f] + (size_t)(b0 + t) * 3 * hw0 * esz, 3 * hw0 * esz,
                                          hipMemcpyDeviceToDevice, s));
            if (bytes_in) HIPCHK(launch_unpack_u8(d_u8, np * hw0, d_up, s));
        } else {
            const char *fr = ims[0] + (size_t)b0 * 3 * hw0 * esz;
            if (unpack) {
                HIPCHK(launch_unpack_u8((const unsigned char *)fr, np * hw0, d_up, s));
            } else {
                x = fr;
                kind = r.in_kind;
            }
        }
        CHK(run_kernels(c, r, g, x, kind, (long)np, nb, net, o.from_triplet(b0, hw0), c->use_graph != 0, s));
    }
    return 0;
}

// ---- a push of a stream: one FlowRequest of n = cams that carries the stream ---------------------------------------------------
// Host push: synchronous -- one upload of the cams frames, the kernels, the download of what was asked for, all on the context's
// stream.  Device push: the kernels alone on the caller's stream.  Both validate first (check_push, the memory kinds, alignment): a
// malformed push leaves the stream as it was.  Whatever fails after that marks the stream broken: the ring slot of the push may
// hold half a frame.
int b2f::stream_push_host(const FlowRequest &r, int *ready)
{
    if (ready) *ready = 0;
    CHK(check_push(r));
    b2f_stream *st = r.stream;
    const FlowOutputs &o = r.o;
    const size_t hw0 = (size_t)st->H0 * st->W0, n = (size_t)st->cams;
    auto kind_of = [](const void *p, size_t bytes) { return p ? mem_kind(p, bytes) : 1; };   // unrequested outputs count as page-locked
    const int k_in = mem_kind(r.im1, n * 3 * hw0 * (st->in_kind == B2F_IN_U8 ? 1 : 4));
    const int k_out[9] = {kind_of(o.flow32, n * 2 * hw0 * 4), kind_of(o.fwd_occ, n * hw0), kind_of(o.bwd_occ, n * hw0), kind_of(o.occ_prob, n * 2 * hw0 * 4),
                          kind_of(o.rgb, n * 3 * hw0), kind_of(o.rgb_max, n * sizeof(double)),
                          kind_of(o.warped, n * 6 * hw0 * (o.warped_kind == B2F_IN_U8 ? 1 : 4)),
                          kind_of(o.photo, n * B2F_PHOTO_WORDS * sizeof(unsigned long long)), kind_of(o.past32, n * 2 * hw0 * 4)};
    bool dev_mem = k_in < 0;
    for (int k : k_out) dev_mem = dev_mem || k < 0;
    if (dev_mem) return fail(std::string(r.who) + ": device memory passed to a host-buffer entry point (use b2f_stream_push_device)");
    const bool is_ready = st->pushed >= 2;
    if (push_host_work(st, r, k_in, k_out) != 0) {
        const std::string msg = api_error();
        (void)hipStreamSynchronize(st->ctx->stream);
        (void)hipGetLastError();
        st->broken = true;
        return fail(msg);
    }
    ++st->pushed;
    if (ready) *ready = is_ready ? 1 : 0;
    return 0;
}

int b2f::stream_push_device(const FlowRequest &r, void *stream, int *ready)
{
    if (ready) *ready = 0;
    CHK(check_push(r));
    b2f_stream *st = r.stream;
    const FlowOutputs &o = r.o;
    if (((uintptr_t)r.im1 | (uintptr_t)o.flow32 | (uintptr_t)o.occ_prob | (uintptr_t)o.fwd_occ | (uintptr_t)o.bwd_occ | (uintptr_t)o.warped |
         (uintptr_t)o.photo | (uintptr_t)o.past32) & 15)
        return fail(std::string(r.who) + ": device buffers must be 16-byte aligned");
    const size_t hw0n = (size_t)st->cams * st->H0 * st->W0, in_bytes = hw0n * 3 * (st->in_kind == B2F_IN_U8 ? 1 : 4);
    const std::pair<const void *, size_t> bufs[8] = {{r.im1, in_bytes}, {o.flow32, hw0n * 8}, {o.occ_prob, hw0n * 8}, {o.fwd_occ, hw0n}, {o.bwd_occ, hw0n},
                                                     {o.warped, 2 * in_bytes}, {o.photo, (size_t)st->cams * B2F_PHOTO_WORDS * sizeof(unsigned long long)},
                                                     {o.past32, hw0n * 8}};
    for (const auto &pb : bufs)
        if (pb.first && mem_kind(pb.first, pb.second) >= 0)
            return fail(std::string(r.who) + ": host memory passed to a device entry point (use b2f_stream_push)");
    const bool is_ready = st->pushed >= 2;
    if (push_device_work(st, r, stream ? (hipStream_t)stream : st->ctx->stream) != 0) {
        const std::string msg = api_error();
        (void)hipGetLastError();
        st->broken = true;
        return fail(msg);
    }
    ++st->pushed;
    if (ready) *ready = is_ready ? 1 : 0;
    return 0;
}

namespace {

// b2f_stream_open (flags = 0) and b2f_stream_open_ex
int stream_open(const char *who, b2f_ctx *c, int cams, int in_kind, int H0, int W0, int flags, b2f_stream **out)
{
    const std::string w(who);
    if (!out) return fail(w + ": null out");
    *out = nullptr;
    if (!c) return fail(w + ": null context");
    if (in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8) return fail(w + ": in_kind must be B2F_IN_UNIT or B2F_IN_U8");
    if (cams < 1) return fail(w + ": a stream serves at least one camera");
    if (H0 < 64 || W0 < 64) return fail(w + ": image smaller than 64 pixels");
    if (!c->g.shipped()) return fail(w + ": streams run on the shipped graph only (this context was made with b2f_init_ex options)");
    if (flags & ~(B2F_STREAM_WARP | B2F_STREAM_PAST)) return fail(w + ": unknown flags (B2F_STREAM_WARP, B2F_STREAM_PAST)");
    if ((flags & B2F_STREAM_PAST) && !c->past_flow)
        return fail(w + ": this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only)");
    if ((flags & B2F_STREAM_WARP) && (long long)H0 * W0 >= (1ll << 28))
        return fail(w + ": images of 2^28 pixels or more are refused (the Q30 sums could overflow)");
    const Geometry g = geometry(c, H0, W0);
    CHK(check_shape(cams, g.fh, g.fw));
    if ((unsigned long long)cams * 3 * g.hw0 > 0x7fffffffull) return fail(w + ": cams x 3 x H0 x W0 exceeds 2^31 - 1 samples");
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<b2f_stream> st(new b2f_stream());
    st->ctx = c; st->cams = cams; st->in_kind = in_kind; st->H0 = H0; st->W0 = W0; st->flags = flags;
    const bool same = g.same, bytes_in = in_kind == B2F_IN_U8;
    const bool warp = (flags & B2F_STREAM_WARP) != 0, past = (flags & B2F_STREAM_PAST) != 0;
    const size_t n = (size_t)cams, hw0 = g.hw0, hw = g.hw;
    st->frame_kind = same ? in_kind : B2F_IN_NORMALIZED;
    st->frame_bytes = same ? n * 3 * hw0 * (bytes_in ? 1 : 4) : n * 3 * hw * 4;
    st->raw_bytes = (warp && !same) ? n * 3 * hw0 * (bytes_in ? 1 : 4) : 0;
    // carve: two passes over the same list, the first one without a base (every pointer stays null) to size the block
    auto carve = [&](char *base) {
        size_t off = 0;
        auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align256(bytes); return p; };
        for (int sl = 0; sl < 3; ++sl)
            for (int l = 3; l <= 7; ++l) st->lvl[sl][l] = (float *)take(n * (size_t)(g.fh >> (l - 1)) * (g.fw >> (l - 1)) * kFeat[l] * 4);
        for (int sl = 0; sl < 3; ++sl) st->frame[sl] = take(st->frame_bytes);
        st->d_u8 = (unsigned char *)take((!same && bytes_in) ? n * 3 * hw0 : 0);
        st->d_up = (float *)take(same ? 0 : n * 3 * hw0 * 4);
        st->d_tmp = (float *)take(same ? 0 : n * 3 * (size_t)H0 * g.fw * 4);
        st->d_flow = (float *)take(n * 2 * hw * 4);
        st->d_occ = (float *)take(n * 2 * hw * 4);
        st->d_est3 = (float *)take(n * 3 * hw * 4);   // three channels: b2f_set_weights may turn a Soft context Hard
        st->d_flow32 = same ? st->d_flow : (float *)take(n * 2 * hw0 * 4);
        st->d_prob = (float *)take(same ? 0 : n * 2 * hw0 * 4);
        st->d_fo = (unsigned char *)take(n * hw0);
        st->d_bo = (unsigned char *)take(n * hw0);
        st->d_rgb = (unsigned char *)take(n * 3 * hw0);
        st->d_max = (double *)take(n * sizeof(double));
        // the pieces of the flags, behind everything a plain stream has
        for (int sl = 0; sl < 3; ++sl) st->raw[sl] = st->raw_bytes ? take(st->raw_bytes) : nullptr;
        st->d_warp = warp ? (void *)take(n * 6 * hw0 * (bytes_in ? 1 : 4)) : nullptr;
        st->d_photo = warp ? (unsigned long long *)take(n * B2F_PHOTO_WORDS * sizeof(unsigned long long)) : nullptr;
        st->d_past = past ? (float *)take(n * 2 * hw * 4) : nullptr;
        st->d_past32 = !past ? nullptr : same ? st->d_past : (float *)take(n * 2 * hw0 * 4);
        return off;
    };
    st->dev_bytes = carve(nullptr);
    if (hipMalloc(&st->dev, st->dev_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(w + ": out of device memory (" + std::to_string(st->dev_bytes >> 20) + " MB for the stream)");
    }
    carve(st->dev);
    // option arena_fill (tests): the block starts as kGuardWord instead of 0, like the arena (carve rounds every piece to 256 bytes)
    if ((c->arena_fill ? hipMemsetD32((hipDeviceptr_t)st->dev, (int)kGuardWord, st->dev_bytes / 4) : hipMemset(st->dev, 0, st->dev_bytes)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(st->dev);
        return fail(w + ": hipMemset failed");
    }
    c->streams.push_back(st.get());
    *out = st.release();
    return 0;
}

// the outputs of b2f_stream_push_warp[_device]: a warp request in the stream's element type, with the past flow when asked for
FlowOutputs push_warp_outputs(const b2f_stream *st, double flow_scale, int own_past, void *warped, unsigned long long *photo, float *flow,
                              float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ, float *past_flow)
{
    FlowOutputs o = warp_outputs(flow_scale, st->in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ);
    o.past32 = past_flow; o.own_past = own_past != 0;
    return o;
}

}  // namespace

extern "C" {

int b2f_stream_open(b2f_ctx *c, int cams, int in_kind, int H0, int W0, b2f_stream **out) try
{
    return stream_open(__func__, c, cams, in_kind, H0, W0, 0, out);
}
B2F_CATCH("b2f_stream_open")

int b2f_stream_open_ex(b2f_ctx *c, int cams, int in_kind, int H0, int W0, int flags, b2f_stream **out) try
{
    return stream_open(__func__, c, cams, in_kind, H0, W0, flags, out);
}
B2F_CATCH("b2f_stream_open_ex")

int b2f_stream_flags(const b2f_stream *st, int *flags) try
{
    if (!st) return fail("b2f_stream_flags: null stream");
    if (flags) *flags = st->flags;
    return 0;
}
B2F_CATCH("b2f_stream_flags")

void b2f_stream_close(b2f_stream *st)
{
    if (!st) return;
    b2f_ctx *c = st->ctx;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();   // pushes may still run, on any stream
    drop_graphs(c);                 // they hold the stream's pointers
    c->streams.erase(std::remove(c->streams.begin(), c->streams.end(), st), c->streams.end());
    if (st->dev) (void)hipFree(st->dev);
    if (st->pin) (void)hipHostFree(st->pin);
    delete st;
}

int b2f_stream_reset(b2f_stream *st) try
{
    if (!st) return fail("b2f_stream_reset: null stream");
    HIPCHK(hipSetDevice(st->ctx->device));
    HIPCHK(hipDeviceSynchronize());   // a device push may still be writing the ring
    st->pushed = 0;
    st->broken = false;
    return 0;
}
B2F_CATCH("b2f_stream_reset")

int b2f_stream_info(const b2f_stream *st, int *cams, int *H0, int *W0, int *in_kind, long long *pushed) try
{
    if (!st) return fail("b2f_stream_info: null stream");
    if (cams) *cams = st->cams;
    if (H0) *H0 = st->H0;
    if (W0) *W0 = st->W0;
    if (in_kind) *in_kind = st->in_kind;
    if (pushed) *pushed = st->pushed;
    return 0;
}
B2F_CATCH("b2f_stream_info")

int b2f_stream_push(b2f_stream *st, const void *frames, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready) try
{
    if (!st) return fail("b2f_stream_push: null stream");
    return stream_push_host(push_request(__func__, st, st->cams, st->in_kind, frames, st->H0, st->W0, {nullptr, flow, occ_prob, fwd_occ, bwd_occ}), ready);
}
B2F_CATCH("b2f_stream_push")

int b2f_stream_push_rgb(b2f_stream *st, const void *frames, double max_norm, int layout, unsigned char *rgb, double *max_used, float *flow,
                        unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready) try
{
    if (!st) return fail("b2f_stream_push_rgb: null stream");
    return stream_push_host(push_request(__func__, st, st->cams, st->in_kind, frames, st->H0, st->W0,
                                         rgb_outputs(rgb, max_used, max_norm, layout, flow, fwd_occ, bwd_occ)), ready);
}
B2F_CATCH("b2f_stream_push_rgb")

int b2f_stream_push_device(b2f_stream *st, const void *dev_frames, float *dev_flow, float *dev_occ_prob, unsigned char *dev_fwd_occ,
                           unsigned char *dev_bwd_occ, void *stream, int *ready) try
{
    if (!st) return fail("b2f_stream_push_device: null stream");
    return stream_push_device(push_request(__func__, st, st->cams, st->in_kind, dev_frames, st->H0, st->W0,
                                           {nullptr, dev_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ}), stream, ready);
}
B2F_CATCH("b2f_stream_push_device")

// ---- pushes of a stream opened with B2F_STREAM_WARP / B2F_STREAM_PAST: the requests of the _warp[_past] and _past entries ----
int b2f_stream_push_warp(b2f_stream *st, const void *frames, double flow_scale, int own_past, void *warped, unsigned long long *photo, float *flow,
                         float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ, float *past_flow, int *ready) try
{
    if (!st) return fail("b2f_stream_push_warp: null stream");
    return stream_push_host(push_request(__func__, st, st->cams, st->in_kind, frames, st->H0, st->W0,
                                         push_warp_outputs(st, flow_scale, own_past, warped, photo, flow, occ_prob, fwd_occ, bwd_occ, past_flow)), ready);
}
B2F_CATCH("b2f_stream_push_warp")

int b2f_stream_push_warp_device(b2f_stream *st, const void *dev_frames, double flow_scale, int own_past, void *dev_warped,
                                unsigned long long *dev_photo, float *dev_flow, float *dev_occ_prob, unsigned char *dev_fwd_occ,
                                unsigned char *dev_bwd_occ, float *dev_past_flow, void *stream, int *ready) try
{
    if (!st) return fail("b2f_stream_push_warp_device: null stream");
    return stream_push_device(push_request(__func__, st, st->cams, st->in_kind, dev_frames, st->H0, st->W0,
                                           push_warp_outputs(st, flow_scale, own_past, dev_warped, dev_photo, dev_flow, dev_occ_prob, dev_fwd_occ,
                                                             dev_bwd_occ, dev_past_flow)), stream, ready);
}
B2F_CATCH("b2f_stream_push_warp_device")

int b2f_stream_push_past(b2f_stream *st, const void *frames, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                         unsigned char *bwd_occ, int *ready) try
{
    if (!st) return fail("b2f_stream_push_past: null stream");
    return stream_push_host(push_request(__func__, st, st->cams, st->in_kind, frames, st->H0, st->W0,
                                         past_outputs(flow, past_flow, occ_prob, fwd_occ, bwd_occ)), ready);
}
B2F_CATCH("b2f_stream_push_past")

int b2f_stream_push_past_device(b2f_stream *st, const void *dev_frames, float *dev_flow, float *dev_past_flow, float *dev_occ_prob,
                                unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream, int *ready) try
{
    if (!st) return fail("b2f_stream_push_past_device: null stream");
    return stream_push_device(push_request(__func__, st, st->cams, st->in_kind, dev_frames, st->H0, st->W0,
                                           past_outputs(dev_flow, dev_past_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ)), stream, ready);
}
B2F_CATCH("b2f_stream_push_past_device")

int b2f_compute_flow(b2f_ctx *c, const float *im1, const float *im2, const float *im3, int H0, int W0, double *flow, unsigned char *fwd_occ,
                     unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, 1, B2F_IN_UNIT, im1, im2, im3, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow")

int b2f_compute_flow_batch(b2f_ctx *c, int n, const float *im1, const float *im2, const float *im3, int H0, int W0, double *flow,
                           unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, B2F_IN_UNIT, im1, im2, im3, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_batch")

int b2f_compute_flow_batch_u8(b2f_ctx *c, int n, const unsigned char *im1, const unsigned char *im2, const unsigned char *im3, int H0,
                              int W0, double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, B2F_IN_U8, im1, im2, im3, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_batch_u8")

int b2f_compute_flow_sequence(b2f_ctx *c, int T, const float *frames, int H0, int W0, double *flow, unsigned char *fwd_occ,
                              unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, B2F_IN_UNIT, frames, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_sequence")

int b2f_compute_flow_sequence_u8(b2f_ctx *c, int T, const unsigned char *frames, int H0, int W0, double *flow, unsigned char *fwd_occ,
                                 unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, B2F_IN_U8, frames, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_sequence_u8")

int b2f_compute_flow_batch_f32(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0, float *flow,
                               float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0, {nullptr, flow, occ_prob, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_batch_f32")

int b2f_compute_flow_sequence_f32(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, float *flow, float *occ_prob,
                                  unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0, {nullptr, flow, occ_prob, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_compute_flow_sequence_f32")

int b2f_compute_flow_batch_rgb(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0, double max_norm,
                               int layout, unsigned char *rgb, double *max_used, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                              rgb_outputs(rgb, max_used, max_norm, layout, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_batch_rgb")

int b2f_compute_flow_sequence_rgb(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, double max_norm, int layout,
                                  unsigned char *rgb, double *max_used, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                 rgb_outputs(rgb, max_used, max_norm, layout, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_sequence_rgb")

int b2f_compute_flow_batch_score(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0, double flow_scale,
                                 const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                 unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                              score_outputs(flow_scale, gt_flow, valid, gt_occ, scores, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_batch_score")

int b2f_compute_flow_sequence_score(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale, const float *gt_flow,
                                    const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                    unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                 score_outputs(flow_scale, gt_flow, valid, gt_occ, scores, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_sequence_score")

int b2f_compute_flow_batch_warp(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0, double flow_scale,
                                void *warped, unsigned long long *photo, float *flow, float *occ_prob, unsigned char *fwd_occ,
                                unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                              warp_outputs(flow_scale, in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_batch_warp")

int b2f_compute_flow_sequence_warp(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale, void *warped,
                                   unsigned long long *photo, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                 warp_outputs(flow_scale, in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_sequence_warp")

int b2f_compute_flow_device(b2f_ctx *c, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3, int H0, int W0,
                            float *dev_flow, float *dev_occ_prob, unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream) try
{
    return compute_flow_device(c, batch_request(__func__, n, in_kind, dev_im1, dev_im2, dev_im3, H0, W0,
                                                {nullptr, dev_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ}), stream);
}
B2F_CATCH("b2f_compute_flow_device")

int b2f_compute_flow_sequence_device(b2f_ctx *c, int T, int in_kind, const void *dev_frames, int H0, int W0, float *dev_flow,
                                     float *dev_occ_prob, unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream) try
{
    return compute_flow_device(c, sequence_request(__func__, T, in_kind, dev_frames, H0, W0,
                                                   {nullptr, dev_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ}), stream);
}
B2F_CATCH("b2f_compute_flow_sequence_device")

// ---- the past flow of a Soft model (skip_ubfs[3]) beside the outputs of the _f32 / _warp / _device entries ----
int b2f_compute_flow_batch_past(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0, float *flow,
                                float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0, past_outputs(flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_batch_past")

int b2f_compute_flow_sequence_past(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, float *flow, float *past_flow,
                                   float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0, past_outputs(flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_sequence_past")

int b2f_compute_flow_device_past(b2f_ctx *c, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3, int H0, int W0,
                                 float *dev_flow, float *dev_past_flow, float *dev_occ_prob, unsigned char *dev_fwd_occ,
                                 unsigned char *dev_bwd_occ, void *stream) try
{
    return compute_flow_device(c, batch_request(__func__, n, in_kind, dev_im1, dev_im2, dev_im3, H0, W0,
                                                past_outputs(dev_flow, dev_past_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ)), stream);
}
B2F_CATCH("b2f_compute_flow_device_past")

int b2f_compute_flow_sequence_device_past(b2f_ctx *c, int T, int in_kind, const void *dev_frames, int H0, int W0, float *dev_flow,
                                          float *dev_past_flow, float *dev_occ_prob, unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ,
                                          void *stream) try
{
    return compute_flow_device(c, sequence_request(__func__, T, in_kind, dev_frames, H0, W0,
                                                   past_outputs(dev_flow, dev_past_flow, dev_occ_prob, dev_fwd_occ, dev_bwd_occ)), stream);
}
B2F_CATCH("b2f_compute_flow_sequence_device_past")

int b2f_compute_flow_batch_warp_past(b2f_ctx *c, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                     double flow_scale, void *warped, unsigned long long *photo, float *flow, float *past_flow, float *occ_prob,
                                     unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_host(c, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                              warp_past_outputs(flow_scale, in_kind, warped, photo, flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_batch_warp_past")

int b2f_compute_flow_sequence_warp_past(b2f_ctx *c, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale, void *warped,
                                        unsigned long long *photo, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                        unsigned char *bwd_occ) try
{
    return compute_flow_host(c, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                 warp_past_outputs(flow_scale, in_kind, warped, photo, flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_compute_flow_sequence_warp_past")

}  // extern "C"
