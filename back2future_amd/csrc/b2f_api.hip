// C-ABI layer of libb2f.so (include/b2f.h): context, weight packing, workspace, the forward
// pass of models/pwc.lua's graph (the host-buffer boundary around it: b2f_pipeline.hip), hipGraph
// capture and per-kernel HIP-event profiling.  The op-level entry points of the kernel tests: b2f_ops.hip.
#include "b2f_ctx.h"

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace b2f;

static thread_local std::string g_err;
namespace b2f {
int api_fail(const std::string &m)
{
    g_err = m;
    return 1;
}
const std::string &api_error() { return g_err; }

// All activations are chunk-planar: [image][C/8][h][w][8].
ConvSeg cp8_seg(const float *ptr, int C, size_t hw)
{
    ConvSeg sgm;
    sgm.ptr = ptr;
    sgm.img_stride = (long)(hw * (size_t)((C + 7) / 8 * 8));
    sgm.chunk_stride = (long)(hw * 8);
    sgm.pix_stride = 8;
    sgm.nchunks = 0;
    return sgm;
}

}  // namespace b2f
static int fail(const std::string &m) { return api_fail(m); }

namespace {

int prof_id(b2f_ctx *c, const char *name)
{
    for (size_t i = 0; i < c->prof_names.size(); ++i)
        if (c->prof_names[i] == name) return (int)i;
    c->prof_names.push_back(name);
    c->prof_ms.push_back(0.0);
    c->prof_n.push_back(0);
    return (int)c->prof_names.size() - 1;
}

hipEvent_t get_event(b2f_ctx *c)
{
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// RAII bracket of one kernel launch with HIP events on the launch stream.
struct Scope {
    b2f_ctx *c;
    hipStream_t s;
    ProfEvent pe;
    bool on;
    Scope(b2f_ctx *c_, hipStream_t s_, const char *name, bool capturing) : c(c_), s(s_), on(c_->profile && !capturing)
    {
        if (on) {
            pe.name = prof_id(c, name);
            pe.a = get_event(c);
            pe.b = get_event(c);
            (void)hipEventRecord(pe.a, s);
        }
    }
    ~Scope()
    {
        if (on) {
            (void)hipEventRecord(pe.b, s);
            c->prof_pending.push_back(pe);
        }
    }
};

int prof_collect(b2f_ctx *c)
{
    for (ProfEvent &pe : c->prof_pending) {
        HIPCHK(hipEventSynchronize(pe.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
        c->prof_ms[pe.name] += ms;
        c->prof_n[pe.name] += 1;
        c->ev_pool.push_back(pe.a);
        c->ev_pool.push_back(pe.b);
    }
    c->prof_pending.clear();
    return 0;
}

// ---- weight packing ------------------------------------------------------------------
// Builds, for every conv of the canonical layout, the K-order the kernels consume:
//   features / inner decoder layers : input channels in order, zero padded to 8
//   decoder layer 1                 : segment 0 = cs[ref][l] (C_l channels),
//                                     segment 1 = cost-volume record (slot order in b2f_internal.h)
// while the Torch order of pwc.lua:308,334 is {cv 162, cs[ref][l] C_l, flow 2}.
int find_conv(const b2f_ctx *c, int kind, int level, int idx);

// B2F_WINO=0 falls back to the direct implicit-GEMM kernel everywhere (A/B runs, parity tests)
bool use_wino()
{
    static const bool on = !(getenv("B2F_WINO") && atoi(getenv("B2F_WINO")) == 0);
    return on;
}

// ---- the conv kernels ------------------------------------------------------------------
// One row per ConvKernel, in the enum's order: everything the packing, the launch and the profile need to know about a kernel.
// Adding a kernel = an enum value, a row here, its condition in `packs` and its rule in choose_kernel.
struct KernelRow {
    const char *tag[2];   // profile_layers rows conv<tag>_<cin>to<cout>_<H>x<W>, by stride - 1 (bench.py parses them)
    const char *cls[2];   // profile class name, by stride - 1; %d = N tiles per block of the layer's fp32 packing
    void (*tiles)(int co, int *nt, int *nblk);
    size_t (*w_floats)(int chunks, int co, int nt, int nblk);
    bool bias;            // the packing ends with nblk * nt * 32 bias floats
    void (*pack)(const float *w, const float *b, int co, int ci, const int *cin_map, int chunks, int nt, int nblk, float *wpk, float *bpk);
    hipError_t (*launch)(const ConvLaunch &, hipStream_t);   // nullptr: a second operand of another kernel's launcher
};
#define TL [](int co, int *nt, int *nblk)
#define WF [](int chunks, int co, int nt, int nblk) -> size_t
#define PK [](const float *w, const float *b, int co, int ci, const int *m, int chunks, int nt, int nblk, float *wpk, float *bpk)
const KernelRow kKernels[K_COUNT] = {
    {{"D1", "D2"}, {"conv3x3_s1_nt%d", "conv3x3_s2_nt%d"}, conv_choose_tiles, WF { return conv_wpk_floats(chunks, nt, nblk); }, true,
     PK { conv_pack_weights(w, b, co, ci, m, chunks, nt, nblk, wpk, bpk); }, launch_conv3x3},
    {{"N2", "N2"}, {"conv3x3_narrow2", "conv3x3_narrow2"}, TL { *nt = 1; *nblk = 1; }, WF { return narrow2_wpk_floats(chunks); }, true,
     PK { narrow2_pack_weights(w, b, ci, m, chunks, wpk, bpk); }, launch_conv_narrow2},
    {{"W2", "W2"}, {"conv3x3_wino_nt%d", "conv3x3_wino_nt%d"}, wino_choose_tiles, WF { return wino_wpk_floats(chunks, nt, nblk); }, true,
     PK { wino_pack_weights(w, b, co, ci, m, chunks, nt, nblk, wpk, bpk); }, launch_conv3x3_wino},
    {{"C16", "C16"}, {"conv3x3_c16_%d", "conv3x3_c16_%d"}, TL { *nt = 1; *nblk = 1; }, WF { return c16_wpk_floats(); }, true,
     PK { c16_pack_weights(w, b, ci, m, wpk, bpk); }, launch_conv3x3_c16},
    {{"S16", "S16"}, {"conv3x3_s2x16_%d", "conv3x3_s2x16_%d"}, TL { *nt = 1; *nblk = 1; }, WF { return c16s2_wpk_floats(); }, true,
     PK { c16s2_pack_weights(w, b, ci, m, wpk, bpk); }, launch_conv3x3_c16s2},
    {{"W4", "W4"}, {"conv3x3_wino4_nt%d", "conv3x3_wino4_nt%d"}, TL { *nt = 2; *nblk = wino4_nblk(co); }, WF { return wino4_wpk_floats(chunks, nblk); }, true,
     PK { wino4_pack_weights(w, b, co, ci, m, chunks, nblk, wpk, bpk); }, launch_conv3x3_wino4},
    {{"E1", "E2"}, {"conv3x3_s1_bf16_%d", "conv3x3_s2_bf16_%d"}, TL { *nt = 2; *nblk = convb_nblk(co); }, WF { return convb_wpk_floats(chunks, co); }, true,
     PK { convb_pack_weights(w, b, co, ci, m, chunks, wpk, bpk); }, launch_conv3x3_bf6},
    {{"L2", "L2"}, {"conv3x3_s2b_%d", "conv3x3_s2b_%d"}, TL { *nt = 1; *nblk = s2b_ntiles(co); }, WF { return s2b_wpk_floats(chunks, co); }, true,
     PK { s2b_pack_weights(w, b, co, ci, m, chunks, wpk, bpk); }, launch_conv3x3_s2b},
    // the n-blocks of more than 32 real outputs; a last block of <= 32 on the F(4x4) single-N-tile kernel, both in one profile row
    {{"V1", "V1"}, {"conv3x3_w1b_%d", "conv3x3_w1b_%d"}, TL { *nt = 2; *nblk = w1b_nblk(co); }, WF { return w1b_wpk_floats(chunks, co); }, true,
     PK { w1b_pack_weights(w, b, co, ci, m, chunks, wpk, bpk); },
     [](const ConvLaunch &L, hipStream_t s) {
         const hipError_t e = launch_conv3x3_w1b(L, s);
         return e == hipSuccess && L.w1b_nblk < w1b_nblk(L.cout) ? launch_conv3x3_wino4_rem(L, s) : e;
     }},
    {{"W6", "W6"}, {"conv3x3_wino6_nt%d", "conv3x3_wino6_nt%d"}, TL { *nt = 2; *nblk = wino6_nblk(co); }, WF { return wino6_wpk_floats(chunks, co); }, true,
     PK { wino6_pack_weights(w, b, co, ci, m, chunks, wpk, bpk); }, launch_conv3x3_wino6},
#if B2F_EXPERIMENTS
    {{nullptr, nullptr}, {nullptr, nullptr}, TL { *nt = 2; *nblk = wino4_nblk(co); }, WF { return wino4s_wpk_floats(chunks, nblk); }, false,
     PK { wino4s_pack_weights(w, co, ci, m, chunks, nblk, wpk); }, nullptr},
    {{nullptr, nullptr}, {nullptr, nullptr}, TL { *nt = 2; *nblk = wino4_nblk(co); }, WF { return wino2s_wpk_floats(chunks, nblk); }, false,
     PK { wino2s_pack_weights(w, co, ci, m, chunks, nblk, wpk); }, nullptr},
#endif
};
#undef TL
#undef WF
#undef PK

// The kernel of a layer by its shape alone: stride-1 layers run F(4x4) from B2F_WINO4_MIN_COUT outputs (default 32; 0 disables it; it
// stores 4 channels at a time), F(2x2) down to B2F_WINO_MIN_COUT (default 16), the direct kernel below; 2 outputs: the VALU kernel,
// which takes one K segment; the two 16-channel layers of the head have kernels of their own.  Stride 2: the direct kernel.
}  // namespace
ConvKernel b2f::base_kernel(int ci, int co, bool stride1, bool two_segments)
{
    static const int min4 = getenv("B2F_WINO4_MIN_COUT") ? atoi(getenv("B2F_WINO4_MIN_COUT")) : 32;
    static const int min2 = getenv("B2F_WINO_MIN_COUT") ? atoi(getenv("B2F_WINO_MIN_COUT")) : 16;
    if (!use_wino()) return K_DIRECT;
    if (ci == 16 && co == (stride1 ? 16 : 32)) return stride1 ? K_C16 : K_C16S2;
    if (!stride1) return K_DIRECT;
    if (co == 2) return two_segments ? K_DIRECT : K_NARROW2;
    if (co < min2) return K_DIRECT;
    return (min4 > 0 && co >= min4 && co % 4 == 0) ? K_WINO4 : K_WINO2;
}
namespace {

// Does a layer carry kernel k's packing?  Its base kernel's always; the optional ones only while an option reads them (the setter
// of such an option repacks when that changes, OptRow::repack).
bool packs(const PackedConv &p, ConvKernel k, bool stride1, const KernelOpts &o)
{
    const bool w4 = p.base == K_WINO4;
    switch (k) {
    case K_BF6: return (p.base == K_DIRECT || (w4 && o.bf16_conv >= 2)) && (p.cout & 3) == 0;
    case K_S2B: return p.base == K_DIRECT && !stride1 && (p.cout & 31) == 0 && p.cout <= 256;
    case K_WINO2: return w4 || p.base == K_WINO2;   // F(4x4) layers: for small maps
    case K_W1B: return w4 && o.wino1d;
    case K_WINO6: return w4 && o.wino6;
#if B2F_EXPERIMENTS
    case K_WINO4S: return w4 && (o.wino4_split || o.wino4_hybrid);   // 1.5x the F(4x4) packing
    case K_WINO2S: return w4 && o.wino2_split;
#endif
    default: return k == p.base;
    }
}

}  // namespace

// Lays the packings of a layer (base, cout and chunks set) out from float offset *total on.  Every packing starts 16-byte aligned
// (conv_narrow2 reads its weights as float4, the split ones are read with dwordx4 loads).
void b2f::place_packings(PackedConv &p, bool stride1, const KernelOpts &o, size_t *total)
{
    for (int k = 0; k < K_COUNT; ++k) {
        if (!packs(p, (ConvKernel)k, stride1, o)) continue;
        PackedConv::Packing &q = p.pk[k];
        kKernels[k].tiles(p.cout, &q.nt, &q.nblk);
        q.w_off = *total = (*total + 3) & ~(size_t)3;
        q.b_off = *total += kKernels[k].w_floats(p.nchunks(), p.cout, q.nt, q.nblk);
        if (kKernels[k].bias) *total += (size_t)q.nblk * q.nt * 32;
    }
}

// Torch weights Co x Ci x 3 x 3 + bias -> every packing place_packings gave the layer
void b2f::fill_packings(const PackedConv &p, const float *w, const float *b, int ci, const int *cin_map, float *host)
{
    for (int k = 0; k < K_COUNT; ++k)
        if (p.has((ConvKernel)k))
            kKernels[k].pack(w, b, p.cout, ci, cin_map, p.nchunks(), p.pk[k].nt, p.pk[k].nblk, host + p.pk[k].w_off, host + p.pk[k].b_off);
}

// The K-order of layer d: sets p.nseg and p.chunks and returns cin_map -- for packed input channel k (segment 0's chunks, then segment 1's)
// the Torch input channel, or -1 (zero weights: channel padding, and the record slots this decoder does not read).
std::vector<int> b2f::layer_cin_map(const ConvDesc &d, bool shipped, PackedConv &p)
{
    std::vector<int> m;
    if (d.kind != KIND_FEAT && d.idx == 1 && shipped) {
        const int Cl = kFeat[d.level];
        const bool has_feat = d.ci >= kND + Cl;          // level-7 flow decoder takes the cost volume only
        const bool has_flow = d.ci == kND + Cl + 2;
        if (has_feat) {
            p.nseg = 2;
            p.chunks[0] = Cl / kCK;
            for (int k = 0; k < Cl; ++k) m.push_back(kND + k);
        } else {
            p.nseg = 1;
        }
        p.chunks[p.nseg - 1] = kCvChunks;   // 21 chunks = 168 floats
        // record slots: 0..79 fwd 0..79 | 80..159 bwd 0..79 | 160 fwd80 | 161 bwd80 | 162,163 ufs | 164,165 ubfs
        const int flow_at = (d.kind == KIND_PAST) ? 164 : 162;   // pwc.lua:334 vs :337
        for (int k = 0; k < kCvRec; ++k) {
            int ci = -1;
            if (k < 80) ci = k;                       // fwd channel k      (Torch cv channel k)
            else if (k < 160) ci = 81 + (k - 80);     // bwd channel k - 80 (Torch cv channel 81 + ..)
            else if (k == 160) ci = 80;
            else if (k == 161) ci = 161;
            else if (has_flow && k >= flow_at && k < flow_at + 2) ci = kND + Cl + (k - flow_at);
            m.push_back(ci);
        }
    } else {
        p.nseg = 1;
        p.chunks[0] = (d.ci + kCK - 1) / kCK;
        for (int k = 0; k < p.chunks[0] * kCK; ++k) m.push_back(k < d.ci ? k : -1);
    }
    return m;
}

namespace {
int pack_all(b2f_ctx *c, const float *flat)
{
    const size_t n = c->lay.size();
    c->packed.assign(n, PackedConv());
    size_t total = 0;
    std::vector<std::vector<int>> maps(n);
    for (size_t i = 0; i < n; ++i) {
        const ConvDesc &d = c->lay[i];
        PackedConv &p = c->packed[i];
        p.cout = d.co;
        // the first conv of a convUnit has stride 2 (the level-1 unit of pwc_skip = 0 has stride 1, pwc.lua:172); the first decoder layer has two K segments
        const bool stride1 = !(d.kind == KIND_FEAT && d.idx == 1 && d.level >= 2);
        p.base = base_kernel(d.ci, d.co, stride1, d.kind != KIND_FEAT && d.idx == 1);
        maps[i] = layer_cin_map(d, c->g.shipped(), p);
        place_packings(p, stride1, *c, &total);
    }
    c->first_w_off = total; total += 27 * 16;
    c->first_b_off = total; total += 16;
    std::vector<float> host(total, 0.f);
    const int id_first = find_conv(c, KIND_FEAT, 2, 1);   // Torch 16 x 3 x 3 x 3 -> [tap (c,ky,kx)][cout]
    if (id_first >= 0 && c->lay[(size_t)id_first].ci == 3 && c->lay[(size_t)id_first].co == 16) {   // (absent with pwc_siamese = 0, 16 -> 16 with pwc_skip = 0)
        const ConvDesc &d = c->lay[(size_t)id_first];
        pack_first_conv(flat + d.w_off, host.data() + c->first_w_off);
        for (int o = 0; o < 16; ++o) host[c->first_b_off + o] = flat[d.b_off + o];
    }
    for (size_t i = 0; i < n; ++i)
        fill_packings(c->packed[i], flat + c->lay[i].w_off, flat + c->lay[i].b_off, c->lay[i].ci, maps[i].data(), host.data());
    if (c->wpk_floats != total) {
        if (c->wpk_dev) HIPCHK(hipFree(c->wpk_dev));
        c->wpk_dev = nullptr;
        HIPCHK(hipMalloc(&c->wpk_dev, total * sizeof(float)));
        c->wpk_floats = total;
    }
    HIPCHK(hipMemcpy(c->wpk_dev, host.data(), total * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int find_conv(const b2f_ctx *c, int kind, int level, int idx)
{
    for (size_t i = 0; i < c->lay.size(); ++i)
        if (c->lay[i].kind == kind && c->lay[i].level == level && c->lay[i].idx == idx) return (int)i;
    return -1;
}

// ---- workspace -------------------------------------------------------------------------
struct Plan {
    int B, H, W;
    bool full;          // full model:forward table (all decoders, image pyramid, image warps)
    bool seq;           // sequence mode: the pyramid holds T = B + 2 frames, triplet b is frames (b, b + 1, b + 2)
    bool stream;        // a push of a stream: the pyramid runs on the B pushed frames, cs[3..7] live in the stream's ring, not in the arena
    bool past;          // the past-flow decoder chain runs: the full table of a Soft model, or a pruned pass asked for Outs::past
    int nimg;           // images of the feature pyramid: 3B (frame-major [3][B]), T = B + 2, or B (stream)
    int fo;             // image offset of a triplet's second / third frame from its first one: B, or 1 in sequence mode
    int rec;            // cost-volume record size in floats
    int h[8], w[8];
    size_t img, tmp, cs[8], U[8], UB[8], cv, d[6], fs, bfs, logits, u2, flow_planar, ds[6], total;
    // option arena_guard (tests): the buffers make_plan took, in order: where each one ends (its own slack included), where the next
    // one may start at the earliest (end rounded to 64 floats + the guard), and its name.  nbuf = 0 without the option.
    enum { kMaxBuf = 40 };
    struct Buf { size_t end, next; const char *name; };
    int nbuf = 0;
    size_t guard = 0;
    Buf buf[kMaxBuf];
};

// guard: option arena_guard.  0 lays the arena out as ever: every buffer rounded up to 64 floats, one behind the other.  Otherwise that many
// floats lie in front of the first buffer and behind every buffer (behind the slack a buffer owns: the record's + 64 is the record's).
Plan make_plan(size_t guard, int B, int H, int W, bool full, bool past_flow, bool seq = false, bool stream = false, bool want_past = false)
{
    static const char *const kCs[8] = {"", "", "cs[2]", "cs[3]", "cs[4]", "cs[5]", "cs[6]", "cs[7]"};
    static const char *const kU[8] = {"", "", "", "U[3]", "U[4]", "U[5]", "U[6]", ""}, *const kUB[8] = {"", "", "", "UB[3]", "UB[4]", "UB[5]", "UB[6]", ""};
    static const char *const kD[6] = {"", "d[1]", "d[2]", "d[3]", "d[4]", "d[5]"}, *const kDs[6] = {"", "", "ds[2]", "ds[3]", "ds[4]", "ds[5]"};
    Plan p;
    p.nbuf = 0;
    p.guard = guard;
    p.B = B; p.H = H; p.W = W;
    p.full = full;
    p.seq = seq;
    p.stream = stream;
    p.past = past_flow && (full || want_past);
    p.nimg = stream ? B : seq ? B + 2 : 3 * B;
    p.fo = seq ? 1 : B;
    p.rec = kCvRec;
    for (int l = 1; l <= 7; ++l) { p.h[l] = H >> (l - 1); p.w[l] = W >> (l - 1); }
    size_t off = guard;
    auto take = [&](size_t n, const char *name) {
        size_t o = off;
        off += (n + 63) & ~(size_t)63;
        if (guard) {
            off += guard;
            p.buf[p.nbuf++] = {o + n, off, name};
        }
        return o;
    };
    p.img = full ? take((size_t)3 * B * H * W * kImgC, "img") : 0;   // packed frames: only the full table needs them
    p.tmp = take((size_t)p.nimg * p.h[2] * p.w[2] * kFeat[2], "tmp");
    for (int l = 2; l <= 7; ++l) p.cs[l] = take((stream && l >= 3) ? 0 : (size_t)p.nimg * p.h[l] * p.w[l] * kFeat[l], kCs[l]);
    for (int l = 3; l <= 6; ++l) p.U[l] = take((size_t)B * p.h[l] * p.w[l] * 2, kU[l]);
    for (int l = 3; l <= 6; ++l) p.UB[l] = p.past ? take((size_t)B * p.h[l] * p.w[l] * 2, kUB[l]) : 0;
    p.cv = take((size_t)B * p.h[3] * p.w[3] * p.rec + 64, "cv");
    const size_t px3 = (size_t)B * p.h[3] * p.w[3];
    for (int i = 1; i <= 5; ++i) p.d[i] = take(px3 * kDec[i], kD[i]);
    p.fs = take(px3 * 8, "fs");       // conv outputs are chunk-planar: 2 channels live in one 8-float chunk
    p.bfs = take(px3 * 8, "bfs");
    p.logits = take(px3 * 8, "logits");
    p.u2 = take(px3 * 4 * 2, "u2");
    p.flow_planar = take((size_t)B * 2 * H * W, "flow_planar");
    // image pyramid ds[f][k], f in {1,3}, k = 2..5 (pwc.lua:148-158): [2][B][H/2^(k-1)][W/2^(k-1)][8]
    for (int k = 2; k <= 5; ++k) p.ds[k] = full ? take((size_t)2 * B * (H >> (k - 1)) * (W >> (k - 1)) * kImgC, kDs[k]) : 0;
    p.total = off;
    return p;
}

}  // namespace
void b2f::drop_gen_out(b2f_ctx *c)
{
    for (float *p : c->gen_out)
        if (p) (void)hipFree(p);
    c->gen_out.clear();
    c->genB = c->genH = c->genW = 0;
}
void b2f::drop_graphs(b2f_ctx *c)
{
    for (auto &g : c->graphs)
        if (g.second) (void)hipGraphExecDestroy(g.second);
    c->graphs.clear();
}
namespace {

int ensure_workspace_floats(b2f_ctx *c, size_t total)
{
    if (total > c->arena_floats) {
        // rare (a larger shape than any before): full device syncs on both sides.  Earlier passes may have run on a
        // caller's stream, and hipMemset is asynchronous on the null stream, which the non-blocking streams the
        // kernels run on do not wait for -- without the second sync the memset could land on top of the first
        // kernels' output (found by tools/soak.py).
        if (c->arena) {
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipFree(c->arena));
            c->arena = nullptr;
            c->arena_floats = 0;
            drop_graphs(c);
        }
        HIPCHK(hipMalloc(&c->arena, total * sizeof(float)));
        HIPCHK(c->arena_fill ? hipMemsetD32((hipDeviceptr_t)c->arena, (int)kGuardWord, total) : hipMemset(c->arena, 0, total * sizeof(float)));
        HIPCHK(hipDeviceSynchronize());
        c->arena_floats = total;
        c->guards.clear();
        c->arena_layout[0] = 0;
    }
    return 0;
}

// Options arena_guard / arena_fill (tests): the arena is in the state of a fresh allocation whenever a pass lays it out differently from the
// pass before -- an arena that has grown once serves smaller shapes and other plans, whose guards would otherwise lie where an earlier
// plan's buffers were -- and the context remembers the plan's guards for b2f_arena_check.  The refill also wipes what the pass before
// left outside the new plan's guards: a stray write is seen only by a b2f_arena_check made after the pass that did it and before the
// next pass with another layout, which is why the tests check after every call.
int prepare_test_arena(b2f_ctx *c, const Plan &p)
{
    const long long key[9] = {1, p.B, p.H, p.W, (p.full ? 1 : 0) | (p.seq ? 2 : 0) | (p.stream ? 4 : 0) | (p.past ? 8 : 0), (long long)p.total, (long long)p.guard,
                              c->arena_fill, (long long)(uintptr_t)c->arena};
    if (!memcmp(key, c->arena_layout, sizeof key)) return 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(c->arena_fill ? hipMemsetD32((hipDeviceptr_t)c->arena, (int)kGuardWord, c->arena_floats) : hipMemset(c->arena, 0, c->arena_floats * sizeof(float)));
    HIPCHK(hipDeviceSynchronize());
    memcpy(c->arena_layout, key, sizeof key);
    c->guards.clear();
    if (p.nbuf) c->guards.push_back({0, p.guard, 0, true, p.buf[0].name});
    for (int i = 0; i < p.nbuf; ++i) c->guards.push_back({p.buf[i].end, p.buf[i].next - p.buf[i].end, i, false, p.buf[i].name});
    return 0;
}

int ensure_workspace(b2f_ctx *c, const Plan &p)
{
    CHK(ensure_workspace_floats(c, p.total));
    if (c->arena_guard | c->arena_fill) CHK(prepare_test_arena(c, p));
    return 0;
}

// ---- one conv launch from the packed table -----------------------------------------------
struct KernelChoice {
    ConvKernel kernel;   // the kernel that runs
    bool f2x2;           // an F(4x4) layer on its F(2x2) packing (kernel = K_WINO2)
    int nsplit;          // ConvLaunch::nsplit
    int w1b_blocks;      // K_W1B: the n-blocks of 64 outputs it computes (ConvLaunch::w1b_nblk)
};

// THE kernel choice: which kernel runs layer p on launch L (sizes, strides, chunk counts and the pointers of every packing the layer has
// filled in: the *_supported predicates read them) under the options o, in a request of cur_batch triplets.  No HIP call.
KernelChoice choose_kernel(const PackedConv &p, const KernelOpts &o, int cur_batch, const ConvLaunch &L)
{
    const int H = L.H, W = L.W;
    // F(4x4) layers fall back to their F(2x2) packing when the launch would leave most of the chip idle.  An F(4x4) block (16 x 32
    // pixels, one per CU) takes about three times as long as an F(2x2) block (8 x 16 pixels) that has its CU to itself and 1.5 times
    // as long as one that shares it with a second block, so compare the number of block rounds each kernel needs on 256 CUs.
    // That rule makes a triplet's result depend (at 1e-6 level) on the batch it is computed in, so it is opt-in (option
    // adaptive_kernels); the default rule looks at the map size only: F(2x2) below wino4_min_pixels.
    bool alt = false, split = false;
    if (p.base == K_WINO4) {
        const PackedConv::Packing &p2 = p.pk[K_WINO2];
        // adaptive_kernels: -1 (default) = per launch for single-triplet calls (the reference's own calling pattern, back2future.lua:73:
        // latency matters and most launches leave the chip half empty), by map size for batches; 0 never, 1 always per launch
        const bool per_launch = o.adaptive_kernels > 0 || (o.adaptive_kernels < 0 && cur_batch == 1);
        if (!per_launch) {
            alt = H * W < o.wino4_min_pixels;
            split = alt && p2.nt == 2 && H * W <= o.wino_split_pixels;
        } else {
            // cost in twentieths of a lone F(2x2) block: F(4x4) block 60; F(2x2) block 20 alone, 40 per pair sharing a CU;
            // F(2x2) block that computes one of the two N tiles only 13 / 26
            const long tiles2 = (long)L.nimg * ((H + 7) / 8) * ((W + 15) / 16);
            const long b4 = (long)L.nimg * ((H + 15) / 16) * ((W + 31) / 32) * p.pk[K_WINO4].nblk;
            const long b2 = tiles2 * p2.nblk, b2s = tiles2 * ((p.cout + 31) / 32);
            const long t4 = 60 * ((b4 + 255) / 256);
            const long t2 = b2 <= 256 ? 20 : 40 * ((b2 + 511) / 512);
            const long t2s = p2.nt != 2 ? t2 : b2s <= 256 ? 13 : 26 * ((b2s + 511) / 512);
            alt = std::min(t2, t2s) < t4;
            split = alt && t2s < t2;
        }
    }
    const ConvKernel mode = alt ? K_WINO2 : p.base;
    KernelChoice ch = {mode, alt, split ? 1 : 0, 0};
    const bool big4 = mode == K_WINO4 && L.stride == 1;   // F(4x4)-class launch: large maps may leave for another kernel
    // the bf16 pipe: direct layers with bf16_conv; bf16_conv >= 2: also F(4x4)-class layers of large maps (2: the 32-output ones, 3: all)
    if (p.has(K_BF6) && ((mode == K_DIRECT && o.bf16_conv) || (big4 && H * W >= o.bf16_conv_min_pixels && ((o.bf16_conv == 2 && p.cout <= 32) || o.bf16_conv >= 3))) &&
        convb_supported(L))
        ch.kernel = K_BF6;
    // stride-2 layers on the bf16 pipe: the loader / consumer kernel.  (Layers of fewer than 64 input channels keep conv3x3_bf6: with four
    // short chunks per tile the loader / consumer block is bound by its weight traffic -- 2 KB per six MFMAs -- 32 -> 64 measured 0.45
    // against 0.43 ms; s2_loader = 2 sends them there too)
    if (mode == K_DIRECT && L.stride == 2 && o.bf16_conv && o.s2_loader && p.has(K_S2B) && (o.s2_loader >= 2 || p.nchunks() >= 8) && s2b_supported(L)) {
        ch.kernel = K_S2B;
        ch.nsplit = o.s2_tile_groups ? 0 : -1;
    }
    if (big4 && ch.kernel == K_WINO4) {
        // wino1d = 1: the n-blocks with more than 32 real outputs on the 1-D Winograd bf16 kernel, a last block of <= 32 outputs on the
        // F(4x4) single-N-tile kernel (half the bf16 kernel's MFMAs would multiply zero padding); 2: every n-block
        const int blocks = o.wino1d >= 2 ? w1b_nblk(p.cout) : p.cout / 64 + (p.cout % 64 > 32 ? 1 : 0);
        if (o.wino1d && p.has(K_W1B) && blocks > 0 && w1b_supported(L)) {
            ch.kernel = K_W1B;
            ch.w1b_blocks = blocks;
        } else if (o.wino6 && p.has(K_WINO6) && H * W >= o.wino6_min_pixels && wino6_supported(L)) {
            // wino6 = 1: Winograd F(6x6) (blocks of 64 outputs, a last block of 32 when the outputs are <= 32 mod 64)
            ch.kernel = K_WINO6;
        }
    }
    return ch;
}

}  // namespace

// Launches layer p, packed at wpk, on the kernel choose_kernel names: the one path of the forward pass (run_conv) and of b2f_op_conv3x3.
// The caller has set L's segments (pointers and strides), output (pointer and strides), sizes, stride, nimg and leaky.
int b2f::launch_layer(b2f_ctx *c, hipStream_t s, bool prof, const PackedConv &p, const float *wpk, const KernelOpts &o, int cur_batch, ConvLaunch &L)
{
    for (int i = 0; i < p.nseg; ++i) L.seg[i].nchunks = p.chunks[i];
    if (p.nseg == 1) L.seg[1] = L.seg[0], L.seg[1].nchunks = 0;
    L.nseg = p.nseg;
    L.cout = p.cout;
    L.Ho = (L.H + 2 - 3) / L.stride + 1;
    L.Wo = (L.W + 2 - 3) / L.stride + 1;
    L.tiles_per_block = o.s2_tiles_per_block;
    L.w4_persist = o.wino4_persistent;
    L.w8 = o.wino8;
    L.bf16_direct = o.bf16_direct;
    auto weights = [&](ConvKernel k) { return p.has(k) ? wpk + p.pk[k].w_off : nullptr; };
    auto bias = [&](ConvKernel k) { return p.has(k) ? wpk + p.pk[k].b_off : nullptr; };
    L.wpk_bf6 = weights(K_BF6); L.bias_bf6 = bias(K_BF6);
    L.wpk_s2b = weights(K_S2B); L.bias_s2b = bias(K_S2B);
    L.wpk_w1b = weights(K_W1B); L.bias_w1b = bias(K_W1B);
    L.wpk_w6 = weights(K_WINO6); L.bias_w6 = bias(K_WINO6);
    const KernelChoice ch = choose_kernel(p, o, cur_batch, L);
    const PackedConv::Packing &q = p.pk[ch.f2x2 ? K_WINO2 : p.base];   // the fp32 packing every launch carries
    L.wpk = wpk + q.w_off;
    L.bias = wpk + q.b_off;
    L.nt = q.nt;
    L.nblk = q.nblk;
    L.nsplit = ch.nsplit;
    L.w1b_nblk = ch.w1b_blocks;
#if B2F_EXPERIMENTS
    if (!ch.f2x2) { L.wpk_split = weights(K_WINO4S); L.wpk_split2 = weights(K_WINO2S); }
    L.w4_hybrid = o.wino4_hybrid;
#endif
    const KernelRow &k = kKernels[ch.kernel];
    char name[48];
    if (c->profile_layers)   // one profile row per (layer shape, map size)
        snprintf(name, sizeof name, "conv%s_%dto%d_%dx%d", (B2F_EXPERIMENTS && ch.kernel == K_C16 && o.bf16_direct) ? "B16" : k.tag[L.stride - 1],
                 p.nchunks() * 8, p.cout, L.H, L.W);
    else
        snprintf(name, sizeof name, k.cls[L.stride - 1], L.nt);
    Scope sc(c, s, name, !prof);
    HIPCHK(k.launch(L, s));
    return 0;
}

namespace {
// All activations are chunk-planar: [image][C/8][h][w][8].
int run_conv(b2f_ctx *c, hipStream_t s, bool cap, int conv_id, const ConvSeg *segs, int nimg, int H, int W,
             int stride, int leaky, float *out)
{
    const PackedConv &p = c->packed[conv_id];
    ConvLaunch L{};
    for (int i = 0; i < p.nseg; ++i) L.seg[i] = segs[i];
    L.out = out;
    L.H = H; L.W = W; L.stride = stride;
    const size_t hwo = (size_t)((H + 2 - 3) / stride + 1) * ((W + 2 - 3) / stride + 1);
    L.out_img_stride = (long)(hwo * ((p.cout + 7) / 8 * 8));
    L.out_chunk_stride = (long)(hwo * 8);
    L.out_pix_stride = 8;
    L.nimg = nimg;
    L.leaky = leaky;
    return launch_layer(c, s, !cap, p, c->wpk_dev, *c, c->cur_batch, L);
}

// decoder(n) of pwc.lua:76-85 at level l; input = {cs[ref][l], cost-volume record}
int run_decoder(b2f_ctx *c, hipStream_t s, bool cap, const Plan &P, const float *ref, int kind, int l, float *out2)
{
    const size_t *dbuf = P.d;
    float *A = c->arena;
    const int h = P.h[l], w = P.w[l], B = P.B;
    const size_t hw = (size_t)h * w;
    const int Cl = kFeat[l];
    const int id1 = find_conv(c, kind, l, 1);
    if (id1 < 0) return fail("decoder not present in this model");
    ConvSeg segs[2];
    const ConvSeg seg_ref = cp8_seg(ref, Cl, hw);
    const ConvSeg seg_cv = cp8_seg(A + P.cv, kCvRec, hw);
    if (c->packed[id1].nseg == 2) { segs[0] = seg_ref; segs[1] = seg_cv; }
    else { segs[0] = seg_cv; segs[1] = seg_cv; }
    CHK(run_conv(c, s, cap, id1, segs, B, h, w, 1, 1, A + dbuf[1]));
    for (int i = 2; i <= 6; ++i) {
        const ConvSeg in = cp8_seg(A + dbuf[i - 1], kDec[i - 1], hw);
        float *o = (i == 6) ? out2 : A + dbuf[i];
        CHK(run_conv(c, s, cap, find_conv(c, kind, l, i), &in, B, h, w, 1, i < 6, o));
    }
    return 0;
}

// Where a pass finds the feature pyramid, per level: pyr = where its nimg images are written; past / ref / fut = the first image of each
// role of the B triplets (image b of a role is triplet b's).  Triplet mode: [3][B] in the arena, the roles B images apart; sequence mode:
// T = B + 2 frames in the arena, the roles one image apart; stream mode: the ring slots of three pushes (pyr[2], the level-2 / fused-head
// map, stays in the arena: nothing reads it after the pyramid).
struct Feat {
    float *pyr[8];
    const float *past[8], *ref[8], *fut[8];
};

Feat make_feat(const b2f_ctx *c, const Plan &P, const StreamPass *sp)
{
    Feat F{};
    for (int l = 2; l <= 7; ++l) {
        const size_t img = (size_t)P.h[l] * P.w[l] * kFeat[l];
        if (sp && l >= 3) {
            F.pyr[l] = sp->pyr[l];
            F.past[l] = sp->past[l]; F.ref[l] = sp->ref[l]; F.fut[l] = sp->fut[l];
        } else {
            F.pyr[l] = c->arena + P.cs[l];
            F.past[l] = F.pyr[l]; F.ref[l] = F.pyr[l] + (size_t)P.fo * img; F.fut[l] = F.pyr[l] + (size_t)2 * P.fo * img;
        }
    }
    return F;
}

// Device outputs of one forward.  Pruned mode (computeFlow): flow / occ / est3 of the finest
// level.  Full mode: the whole output table of pwc.lua:459-489, per level l = 3..7 (index l):
// skip_ufs, skip_ubfs (Soft), skip_occs, iws[1], iws[3], all planar at 4h_l x 4w_l.
struct Outs {
    float *flow = nullptr, *occ = nullptr, *est3 = nullptr;
    float *past = nullptr;   // pruned mode, Soft only: skip_ubfs[3], B x 2 x H x W planar (runs the past-flow decoder chain)
    float *t_ufs[8] = {nullptr}, *t_ubfs[8] = {nullptr}, *t_occ[8] = {nullptr}, *t_iw1[8] = {nullptr}, *t_iw3[8] = {nullptr};
};

// The computeFlow graph: pruned to the live set or, with P.full, the
// complete model:forward of models/pwc.lua.  With P.seq the input is T = B + 2 frames (T x 3 x H x W) and the pyramid
// runs on each frame once; from the cost volume on, the launches are those of B triplets, which read their frames
// through base pointers P.fo images apart.  With sp (a push of a stream) the input is the B = cams pushed frames, the pyramid writes
// the ring slot of the push, and the rest -- only when the stream holds three frames -- reads the slots of three pushes (make_feat).
int forward_impl(b2f_ctx *c, hipStream_t s, bool cap, const void *dev_in, int in_kind, const Plan &P, const Outs &O, const StreamPass *sp = nullptr)
{
    c->cur_batch = c->req_batch > 0 ? c->req_batch : P.B;
    float *A = c->arena;
    const Feat F = make_feat(c, P, sp);
    const int B = P.B;
    const bool full = P.full, past = P.past;
    const int unit = in_kind == B2F_IN_UNIT;
    if (full) {   // the packed frames are only needed for the image pyramid / image warps of the full table
        Scope sc(c, s, "pack_input", cap);
        HIPCHK(launch_pack_input((const float *)dev_in, unit, B, P.H, P.W, A + P.img, s));
    }
    // siamese feature pyramid, the three frames batched (shared weights, pwc.lua:169-211); P.nimg images
    // (the head kernel reads the c16 / c16s2 packings of its two layers: B2F_WINO=0 packs them for the direct kernel instead)
    const int head_id1 = find_conv(c, KIND_FEAT, 2, 2), head_id2 = find_conv(c, KIND_FEAT, 3, 1);
    const bool head_fused = c->bf16_direct >= 2 && P.h[2] >= 4 && P.w[2] >= 4 && head_id1 >= 0 && head_id2 >= 0 &&
                            c->packed[(size_t)head_id1].base == K_C16 && c->packed[(size_t)head_id2].base == K_C16S2;   // level-2 conv 2 + level-3 conv 1 as one streaming kernel; cs[2] then holds the 32-channel level-3 map
    for (int l = 2; l <= 7; ++l) {
        const int hi = P.h[l - 1], wi = P.w[l - 1], ho = P.h[l], wo = P.w[l];
        const int Ci = (l == 2) ? kImgC : kFeat[l - 1], Co = kFeat[l];
        if (l == 2 && (P.seq || sp)) {
            Scope sc(c, s, "conv_first_seq", cap);
            HIPCHK(launch_conv_first_seq(dev_in, in_kind, P.nimg, P.H, P.W, c->wpk_dev + c->first_w_off, c->wpk_dev + c->first_b_off,
                                         A + P.tmp, s));
        } else if (l == 2) {
            Scope sc(c, s, "conv_first", cap);
            HIPCHK(launch_conv_first((const float *)dev_in, unit, B, P.H, P.W, c->wpk_dev + c->first_w_off,
                                     c->wpk_dev + c->first_b_off, A + P.tmp, s));
        } else if (l == 3 && head_fused) {   // conv 1 of level 3 ran inside the fused head: its output sits in the (otherwise unused) cs[2] region
            const ConvSeg in2f = cp8_seg(A + P.cs[2], Co, (size_t)ho * wo);
            CHK(run_conv(c, s, cap, find_conv(c, KIND_FEAT, l, 2), &in2f, P.nimg, ho, wo, 1, 1, F.pyr[l]));
            continue;
        } else {
            const ConvSeg in1 = cp8_seg(F.pyr[l - 1], Ci, (size_t)hi * wi);
            CHK(run_conv(c, s, cap, find_conv(c, KIND_FEAT, l, 1), &in1, P.nimg, hi, wi, 2, 1, A + P.tmp));
        }
        if (l == 2 && head_fused) {   // level-2 conv 2 + level-3 conv 1 in one streaming kernel (b2f_head.hip)
            const PackedConv::Packing &p1 = c->packed[(size_t)head_id1].pk[K_C16], &p2 = c->packed[(size_t)head_id2].pk[K_C16S2];
            HeadLaunch hl;
            hl.in = A + P.tmp; hl.in_img_stride = (long)((size_t)ho * wo * 16); hl.in_chunk_stride = (long)((size_t)ho * wo * 8); hl.in_pix_stride = 8;
            hl.H1 = ho; hl.W1 = wo;
            hl.w1 = c->wpk_dev + p1.w_off; hl.b1 = c->wpk_dev + p1.b_off; hl.w2 = c->wpk_dev + p2.w_off; hl.b2 = c->wpk_dev + p2.b_off;
            hl.out = A + P.cs[2];
            hl.Ho = P.h[3]; hl.Wo = P.w[3]; hl.nimg = P.nimg;
            hl.out_img_stride = (long)((size_t)hl.Ho * hl.Wo * 32); hl.out_chunk_stride = (long)((size_t)hl.Ho * hl.Wo * 8); hl.out_pix_stride = 8;
            char hname[48];
            snprintf(hname, sizeof hname, c->profile_layers ? "convH16_16to32_%dx%d" : "conv_head16_bf16", ho, wo);
            Scope sc(c, s, hname, cap);
            HIPCHK(launch_conv_head16(hl, s));
            continue;
        }
        const ConvSeg in2 = cp8_seg(A + P.tmp, Co, (size_t)ho * wo);
        CHK(run_conv(c, s, cap, find_conv(c, KIND_FEAT, l, 2), &in2, P.nimg, ho, wo, 1, 1, F.pyr[l]));
    }
    if (sp && !sp->ready) return 0;   // pushes 1 and 2 of a stream: the features are in the ring, there is no triplet yet
    if (full) {
        // image pyramid of frames 1 and 3 for the warped-image outputs (pwc.lua:148-158);
        // ds[k] holds [frame 1 | frame 3], level 1 is the packed input itself
        Scope sc(c, s, "avgpool2", cap);
        const size_t img_f = (size_t)B * P.H * P.W * kImgC;
        for (int f = 0; f < 2; ++f) {
            const float *src = A + P.img + (size_t)(f == 0 ? 0 : 2) * img_f;
            for (int k = 2; k <= 5; ++k) {
                const int hk = P.H >> (k - 2), wk = P.W >> (k - 2);
                float *dst = A + P.ds[k] + (size_t)f * B * (hk / 2) * (wk / 2) * kImgC;
                HIPCHK(launch_avgpool2_nhwc(src, B, hk, wk, kImgC, dst, s));
                src = dst;
            }
        }
    }
    for (int l = 7; l >= 3; --l) {   // pwc.lua:237
        const int h = P.h[l], w = P.w[l], Cl = kFeat[l];
        const size_t hw = (size_t)h * w;
        CorrLaunch cl;
        cl.ref = F.ref[l];
        cl.nbr_fut = F.fut[l];
        cl.nbr_past = F.past[l];
        cl.img_stride = (long)(hw * Cl);
        cl.chunk_stride = (long)(hw * 8);
        cl.pix_stride = 8;
        cl.flow = (l < 7) ? A + P.U[l] : nullptr;
        cl.flow_b = (l < 7 && past) ? A + P.UB[l] : nullptr;
        cl.k = (float)(20.0 / std::pow(2.0, l - 1));   // nn.MulConstant(20*(f-ref)/2^(l-2)) one level up, pwc.lua:404
        cl.out = A + P.cv;
        cl.out_img_stride = (long)(hw * kCvRec);
        cl.out_chunk_stride = (long)(hw * 8);
        cl.out_pix_stride = 8;
        cl.B = B; cl.C = Cl; cl.h = h; cl.w = w;
        cl.variant = c->corr_variant;
        cl.ablate = c->corr_ablate;
        {
            char cname[48];
            snprintf(cname, sizeof cname, c->profile_layers ? "warp_costvol_%dx%d" : "warp_costvol", h, w);
            Scope sc(c, s, cname, cap);
            HIPCHK(launch_warp_costvol(cl, s));
        }
        // occlusion decoder + SpatialSoftMax + nearest x4 (pwc.lua:288-321); dead below level 3 unless full
        float *occ_out = full ? O.t_occ[l] : (l == 3 ? O.occ : nullptr);
        float *occ_out2 = (!full && l == 3 && c->past_flow) ? O.est3 : nullptr;   // Soft: est[3] = skip_occs[3]
        if (occ_out || occ_out2) {
            // (round 3 ran this decoder on a side stream beside the flow decoder: both chains are chip-filling persistent
            // kernels, measured no gain, and the second set of intermediates cost a third of the arena -- removed in round 4)
            CHK(run_decoder(c, s, cap, P, F.ref[l], KIND_OCC, l, A + P.logits));
            {
                Scope sc(c, s, "softmax_nearest4", cap);
                if (occ_out) HIPCHK(launch_softmax_nearest4_planar(A + P.logits, 8, B, h, w, occ_out, s));
                if (occ_out2) HIPCHK(launch_softmax_nearest4_planar(A + P.logits, 8, B, h, w, occ_out2, s));
            }
        }
        CHK(run_decoder(c, s, cap, P, F.ref[l], KIND_FLOW, l, A + P.fs));
        if (past) CHK(run_decoder(c, s, cap, P, F.ref[l], KIND_PAST, l, A + P.bfs));
        // upsampling (pwc.lua:359-390): ufs = bilinear x2; skip_ufs = a second bilinear x2
        float *skip_f = full ? O.t_ufs[l] : (l == 3 ? (O.flow ? O.flow : A + P.flow_planar) : nullptr);
        {
            Scope sc(c, s, "upsample_flow2x", cap);
            float *u = (l > 3) ? A + P.U[l - 1] : A + P.u2;
            HIPCHK(launch_upsample_flow2x(A + P.fs, 8, B, h, w, u, s));
            if (skip_f) HIPCHK(launch_upsample_flow2x_planar(u, 2, B, 2 * h, 2 * w, skip_f, s));
            if (past) {
                // the past flow of level 3 has no next level: its x2 goes through the second half of u2's slot
                float *ub = (l > 3) ? A + P.UB[l - 1] : A + P.d[1];
                HIPCHK(launch_upsample_flow2x(A + P.bfs, 8, B, h, w, ub, s));
                float *skip_b = full ? O.t_ubfs[l] : (l == 3 ? O.past : nullptr);
                if (skip_b) HIPCHK(launch_upsample_flow2x_planar(ub, 2, B, 2 * h, 2 * w, skip_b, s));
            }
        }
        if (full) {
            // warped images iws[f][l] = warp(ds[f][l-2], skip_u(b)fs[l] * 20(f-2)/2^(l-3))  (pwc.lua:422-446)
            Scope sc(c, s, "warp_image", cap);
            const int k = l - 2;   // pyramid level of the image (1 = full resolution)
            const int hk = 4 * h, wk = 4 * w;
            const size_t img_f = (size_t)B * hk * wk * kImgC;
            const float *im1 = (k == 1) ? A + P.img : A + P.ds[k];
            const float *im3 = (k == 1) ? A + P.img + 2 * img_f : A + P.ds[k] + img_f;
            const float kk = (float)(20.0 / std::pow(2.0, l - 3));
            const float *fl1 = (past && O.t_ubfs[l]) ? O.t_ubfs[l] : O.t_ufs[l];
            if (O.t_iw1[l]) HIPCHK(launch_warp_image_planar(im1, fl1, -kk, B, hk, wk, O.t_iw1[l], s));
            if (O.t_iw3[l]) HIPCHK(launch_warp_image_planar(im3, O.t_ufs[l], kk, B, hk, wk, O.t_iw3[l], s));
        }
    }
    if (!full && O.est3 && !c->past_flow && (P.seq || sp)) {
        // frame b of the sequence, or camera b's frame of two pushes ago, is the first frame of triplet b
        Scope sc(c, s, "warp_image_seq", cap);
        HIPCHK(launch_warp_input_seq(sp ? sp->frame_past : dev_in, sp ? sp->frame_kind : in_kind, O.flow ? O.flow : A + P.flow_planar, -20.0f, B,
                                     P.H, P.W, O.est3, s));
    } else if (!full && O.est3 && !c->past_flow) {
        // Hard: est[3] = iws[1][3] = warp(I1, skip_ufs[3] * 20*(1-2)/2^0)  (pwc.lua:422-446,459-489)
        Scope sc(c, s, "warp_image", cap);
        HIPCHK(launch_warp_input_planar((const float *)dev_in, unit, 0, O.flow ? O.flow : A + P.flow_planar, -20.0f, B, P.H, P.W,
                                        O.est3, s));
    }
    return 0;
}

}  // namespace
int b2f::find_conv_id(const b2f_ctx *c, int kind, int level, int idx) { return find_conv(c, kind, level, idx); }
int b2f::run_conv_layer(b2f_ctx *c, hipStream_t s, bool cap, int conv_id, const ConvSeg *segs, int nimg, int H, int W, int stride,
                        int leaky, float *out)
{
    if (conv_id < 0) return fail("b2f: layer not present in this model");
    return run_conv(c, s, cap, conv_id, segs, nimg, H, W, stride, leaky, out);
}
// The generic executor lays the arena out itself (graph_run's Bump): no plan's guards, and the next plan refills.  With arena_guard /
// arena_fill its layout is treated as prepare_test_arena treats a plan: refilled whenever it differs from the pass before -- another
// shape, guard width, fill, arena, or a plan in between -- and its guards remembered, by role and level, for b2f_arena_check.
int b2f::ensure_arena(b2f_ctx *c, size_t floats, std::vector<GraphBuf> &&bufs, int B, int H, int W)
{
    CHK(ensure_workspace_floats(c, floats));
    if (!(c->arena_guard | c->arena_fill)) {
        c->guards.clear();
        c->arena_layout[0] = 0;
        return 0;
    }
    const long long key[9] = {2, B, H, W, 0, (long long)floats, (long long)c->arena_guard, c->arena_fill, (long long)(uintptr_t)c->arena};
    if (!memcmp(key, c->arena_layout, sizeof key)) return 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(c->arena_fill ? hipMemsetD32((hipDeviceptr_t)c->arena, (int)kGuardWord, c->arena_floats) : hipMemset(c->arena, 0, c->arena_floats * sizeof(float)));
    HIPCHK(hipDeviceSynchronize());
    memcpy(c->arena_layout, key, sizeof key);
    c->guards.clear();
    c->graph_bufs = std::move(bufs);
    const std::vector<GraphBuf> &gb = c->graph_bufs;
    if (!gb.empty()) c->guards.push_back({0, (size_t)c->arena_guard, 0, true, gb[0].name.c_str()});
    for (size_t i = 0; i < gb.size(); ++i) c->guards.push_back({gb[i].end, gb[i].next - gb[i].end, (int)i, false, gb[i].name.c_str()});
    return 0;
}
int b2f::check_shape(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return fail("b2f: non-positive shape");
    if (H % 64 || W % 64) return fail("b2f: H and W must be multiples of 64 (7 pyramid levels, back2future.lua:54-67)");
    return 0;
}
namespace {

bool parse_random(const char *name, bool *past, unsigned long long *seed, float *gain)
{
    if (strncmp(name, "random:", 7) != 0) return false;
    std::string s(name + 7);
    std::vector<std::string> parts;
    size_t pos = 0;
    while (true) {
        size_t q = s.find(':', pos);
        parts.push_back(s.substr(pos, q == std::string::npos ? q : q - pos));
        if (q == std::string::npos) break;
        pos = q + 1;
    }
    if (parts[0] == "hard") *past = false;
    else if (parts[0] == "soft") *past = true;
    else return false;
    *seed = 2;   // manualSeed default, opts.lua:27
    *gain = 1.f;
    if (parts.size() > 1 && !parts[1].empty()) *seed = strtoull(parts[1].c_str(), nullptr, 10);
    if (parts.size() > 2 && !parts[2].empty()) *gain = strtof(parts[2].c_str(), nullptr);
    return true;
}

bool ends_with(const std::string &s, const char *suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

int install_weights(b2f_ctx *c, const float *flat, long long n, bool past)
{
    GraphOpts g = c->g;
    g.past_flow = past;
    if (n != param_count(g)) return fail("b2f: weight count does not match the architecture");
    // captured graphs hold the packed-weight pointers and the Hard / Soft topology of the moment they were captured
    HIPCHK(hipDeviceSynchronize());
    drop_graphs(c);
    drop_gen_out(c);
    if (c->w_dev && (c->nparams != n)) { HIPCHK(hipFree(c->w_dev)); c->w_dev = nullptr; }
    c->past_flow = past;
    c->g = g;
    c->nparams = n;
    long long t = 0;
    c->lay = weight_layout(g, &t);
    if (!c->w_dev) HIPCHK(hipMalloc(&c->w_dev, (size_t)n * sizeof(float)));
    HIPCHK(hipMemcpy(c->w_dev, flat, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return pack_all(c, flat);
}

// ---- options ---------------------------------------------------------------------------
// One row per b2f_set_option / b2f_get_option key; b2f_init seeds the OPT_ENV ones from B2F_<NAME IN CAPITALS>.
enum {
    OPT_ENV = 1,        // seeded from the environment at b2f_init
    OPT_SYNC = 2,       // a different kernel mix: setting it synchronises the device and drops the captured graphs, which hold the old one
    OPT_EXP_ONLY = 4,   // selects a kernel of tools/experiments/csrc: the product build has no such option (not seeded, only 0 accepted)
    OPT_ARENA = 8,      // lays out or fills the arena differently: setting it synchronises the device, frees the arena and drops the captured graphs
};
struct OptRow {
    const char *name;
    int b2f_ctx::*member;
    int flags;
    int repack;         // > 0: an optional packing exists only while an option of this group reads it (reads_packing); a set that changes that repacks
};
const OptRow kOptions[] = {
    {"use_graph", &b2f_ctx::use_graph, OPT_ENV, 0},
    {"host_graph", &b2f_ctx::host_graph, OPT_ENV, 0},
    {"profile", &b2f_ctx::profile, OPT_ENV, 0},
    {"profile_layers", &b2f_ctx::profile_layers, OPT_ENV, 0},
    {"corr_variant", &b2f_ctx::corr_variant, OPT_ENV | OPT_SYNC, 0},
    {"corr_ablate", &b2f_ctx::corr_ablate, OPT_ENV | OPT_SYNC, 0},
    {"bf16_direct", &b2f_ctx::bf16_direct, OPT_ENV | OPT_SYNC, 0},
    {"bf16_conv", &b2f_ctx::bf16_conv, OPT_ENV | OPT_SYNC, 1},
    {"bf16_conv_min_pixels", &b2f_ctx::bf16_conv_min_pixels, OPT_SYNC, 0},
    {"wino1d", &b2f_ctx::wino1d, OPT_ENV | OPT_SYNC, 2},
    {"wino6", &b2f_ctx::wino6, OPT_ENV | OPT_SYNC, 3},
    {"wino6_min_pixels", &b2f_ctx::wino6_min_pixels, OPT_ENV | OPT_SYNC, 0},
    {"wino2_split", &b2f_ctx::wino2_split, OPT_ENV | OPT_SYNC | OPT_EXP_ONLY, 4},
    {"wino4_split", &b2f_ctx::wino4_split, OPT_ENV | OPT_SYNC | OPT_EXP_ONLY, 5},
    {"wino4_hybrid", &b2f_ctx::wino4_hybrid, OPT_ENV | OPT_SYNC | OPT_EXP_ONLY, 5},
    {"s2_tiles_per_block", &b2f_ctx::s2_tiles_per_block, OPT_ENV | OPT_SYNC, 0},
    {"wino4_persistent", &b2f_ctx::wino4_persistent, OPT_ENV | OPT_SYNC, 0},
    {"s2_loader", &b2f_ctx::s2_loader, OPT_ENV | OPT_SYNC, 0},
    {"s2_tile_groups", &b2f_ctx::s2_tile_groups, OPT_ENV | OPT_SYNC, 0},
    {"wino_split_pixels", &b2f_ctx::wino_split_pixels, OPT_ENV | OPT_SYNC, 0},
    {"wino8", &b2f_ctx::wino8, OPT_ENV | OPT_SYNC, 0},
    {"wino4_min_pixels", &b2f_ctx::wino4_min_pixels, OPT_ENV | OPT_SYNC, 0},
    {"adaptive_kernels", &b2f_ctx::adaptive_kernels, OPT_ENV | OPT_SYNC, 0},
    {"op_wino_split", &b2f_ctx::op_wino_split, OPT_ENV, 0},
    {"op_gradw_partials", &b2f_ctx::op_gradw_partials, OPT_ENV, 0},
    {"op_hole_fill", &b2f_ctx::op_hole_fill, 0, 0},
    {"host_subbatch_pixels", nullptr, OPT_ENV, 0},   // long long b2f_ctx::host_subbatch_pixels
    {"host_threads", &b2f_ctx::host_threads, OPT_ENV, 0},
    {"host_u8", &b2f_ctx::host_u8, OPT_ENV, 0},
    {"host_ramp", &b2f_ctx::host_ramp, OPT_ENV, 0},
    {"debug_fail_next", &b2f_ctx::debug_fail_next, 0, 0},
    {"arena_guard", &b2f_ctx::arena_guard, OPT_ARENA, 0},
    {"arena_fill", &b2f_ctx::arena_fill, OPT_ARENA, 0},
};

const OptRow *find_option(const char *key)
{
    for (const OptRow &r : kOptions)
        if (!strcmp(key, r.name)) return &r;
    return nullptr;
}

// does an option of repack group `group` read the group's optional packing?  (F(4x4)-class layers carry the bf16 direct packing only while
// bf16_conv >= 2; the other packings while an option of their group is not 0)
bool reads_packing(const b2f_ctx *c, int group)
{
    for (const OptRow &r : kOptions)
        if (r.repack == group && (r.member == &b2f_ctx::bf16_conv ? c->*r.member >= 2 : c->*r.member != 0)) return true;
    return false;
}

// A value that names an experiment kernel, not in the product build: refused by b2f_set_option with this text; from the environment b2f_init
// warns and keeps the default (an A/B run driven by the environment would otherwise time the default kernel under another label).  nullptr = fine.
const char *experiment_value(const OptRow &r, int value)
{
    if (B2F_EXPERIMENTS) return nullptr;
    if (r.member == &b2f_ctx::corr_variant && (value == 2 || value == 4 || value == 6 || value == 8))
        return "b2f_set_option: corr_variant 2 / 4 / 6 / 8 are experiment kernels: build with `python -m back2future_amd.build --experiments`";
    if (r.member == &b2f_ctx::bf16_direct && value == 1)
        return "b2f_set_option: bf16_direct = 1 (the 16 -> 16 layer alone on the bf16 pipe) is an experiment: build with `python -m back2future_amd.build --experiments`";
    return nullptr;
}

}  // namespace

// ======================================================================================
extern "C" {

const char *b2f_last_error(void) { return g_err.c_str(); }
int b2f_version(void) { return 1015; }

long long b2f_param_count(int past_flow) { return param_count(past_flow != 0); }

int b2f_random_weights(unsigned long long seed, int past_flow, float gain, float *out, long long n) try
{
    if (!out || n != param_count(past_flow != 0)) return fail("b2f_random_weights: bad buffer size");
    random_weights(seed, past_flow != 0, gain, out);
    return 0;
}
B2F_CATCH("b2f_random_weights")

int b2f_load_t7(const char *path, float *out, long long cap, long long *n, int *past_flow) try
{
    std::vector<float> flat;
    bool past = false;
    std::string err;
    if (!path) return fail("b2f_load_t7: null path");
    if (!load_t7(path, flat, past, err)) return fail("b2f_load_t7: " + err);
    if (n) *n = (long long)flat.size();
    if (past_flow) *past_flow = past ? 1 : 0;
    if (out) {
        if (cap < (long long)flat.size()) return fail("b2f_load_t7: output buffer too small");
        memcpy(out, flat.data(), flat.size() * sizeof(float));
    }
    return 0;
}
B2F_CATCH("b2f_load_t7")

int b2f_load_t7_ex(const char *path, const char *graph_opts, float *out, long long cap, long long *n, char *opts_out, int opts_cap) try
{
    if (!path) return fail("b2f_load_t7_ex: null path");
    GraphOpts g;
    std::string err;
    if (!parse_graph_opts(graph_opts, g, err)) return fail("b2f_load_t7_ex: " + err);
    std::vector<float> flat;
    if (!load_t7_ex(path, g, !(graph_opts && *graph_opts), flat, err)) return fail("b2f_load_t7_ex: " + err);
    if (n) *n = (long long)flat.size();
    if (opts_out && opts_cap > 0) {
        const std::string t = graph_opts_string(g);
        if ((int)t.size() + 1 > opts_cap) return fail("b2f_load_t7_ex: option buffer too small");
        memcpy(opts_out, t.c_str(), t.size() + 1);
    }
    if (out) {
        if (cap < (long long)flat.size()) return fail("b2f_load_t7_ex: output buffer too small");
        memcpy(out, flat.data(), flat.size() * sizeof(float));
    }
    return 0;
}
B2F_CATCH("b2f_load_t7_ex")

int b2f_init(const char *name_or_path, int device, b2f_ctx **out) { return b2f_init_ex(name_or_path, device, nullptr, out); }

int b2f_init_ex(const char *name_or_path, int device, const char *graph_opts, b2f_ctx **out) try
{
    if (!out) return fail("b2f_init: null out");
    *out = nullptr;
    GraphOpts g;
    {
        std::string err;
        if (!parse_graph_opts(graph_opts, g, err)) return fail("b2f_init: " + err);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("b2f_init: no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("b2f_init: bad device ordinal");
    HIPCHK(hipSetDevice(device));
    const char *name = name_or_path ? name_or_path : "Ours-Soft-ft-KITTI";   // back2future.lua:98
    std::vector<float> flat;
    bool past = false;
    unsigned long long seed = 2;
    float gain = 1.f;
    if (parse_random(name, &past, &seed, &gain)) {
        g.past_flow = past;
        flat.resize((size_t)param_count(g));
        random_weights(seed, g, gain, flat.data());
    } else {
        std::string path = name;
        if (path == "Ours-Hard") path = "models/RoamingImages_H.t7";                      // :100-102
        else if (path == "Ours-Soft-ft-KITTI") path = "models/RoamingImages_H_KITTI_S.t7";   // :104-106
        else if (path == "Ours-Soft-ft-Sintel") path = "models/RoamingImages_H_Sintel_S.t7"; // :108-110
        if (ends_with(path, ".t7")) {
            // without graph options the shape (win, levels, skip) is read from the file; with them the file must be that graph
            std::string err;
            if (!load_t7_ex(path, g, !(graph_opts && *graph_opts), flat, err)) return fail("b2f_init: " + err);
            past = g.past_flow;
        } else if (ends_with(path, ".b2fw")) {
            FILE *f = fopen(path.c_str(), "rb");
            if (!f) return fail("b2f_init: cannot open " + path);
            fseek(f, 0, SEEK_END);
            const long sz = ftell(f);
            fseek(f, 0, SEEK_SET);
            flat.resize((size_t)sz / 4);
            const size_t rd = fread(flat.data(), 4, flat.size(), f);
            fclose(f);
            if (rd != flat.size()) return fail("b2f_init: short read on " + path);
            GraphOpts gp = g, gn = g;
            gp.past_flow = true; gn.past_flow = false;
            if ((long long)flat.size() == param_count(gp)) past = true;
            else if ((long long)flat.size() == param_count(gn)) past = false;
            else return fail("b2f_init: " + path + " does not hold a parameter set of this graph (with or without past-flow decoders)");
        } else {
            return fail(std::string("b2f_init: unknown model '") + name + "'");
        }
    }
    b2f_ctx *c = new b2f_ctx();
    c->device = device;
    c->g = g;
    {   // defaults of the tuning options may come from the environment; read here once, never on the hot path
        // B2F_<OPTION NAME IN CAPITALS> seeds the option of that name (b2f_set_option keys); a value that is set but not a
        // number (B2F_PROFILE_LAYERS=yes, or empty) counts as 1
        auto env_int = [](const std::string &k, long long dflt) {
            const char *v = getenv(k.c_str());
            if (!v) return dflt;
            char *end = nullptr;
            const long long x = strtoll(v, &end, 10);
            return end == v ? 1ll : x;
        };
        if (!use_wino()) { c->bf16_conv = 0; c->bf16_direct = 0; }   // B2F_WINO=0: every layer on the direct fp32-MFMA kernel (bit-exact fmaf chains)
        c->corr_variant = (int)env_int("B2F_CORR_LAT", c->corr_variant);   // the round-1 name of B2F_CORR_VARIANT
        for (const OptRow &r : kOptions) {
            if (!(r.flags & OPT_ENV) || ((r.flags & OPT_EXP_ONLY) && !B2F_EXPERIMENTS)) continue;
            std::string k = std::string("B2F_") + r.name;
            for (char &ch : k) ch = (char)toupper((unsigned char)ch);
            if (!r.member) {
                c->host_subbatch_pixels = env_int(k, c->host_subbatch_pixels);
                continue;
            }
            c->*r.member = (int)env_int(k, c->*r.member);
            if (experiment_value(r, c->*r.member)) {
                const bool corr = r.member == &b2f_ctx::corr_variant;
                fprintf(stderr, "b2f_init: %s=%d is an experiment%s (build with `python -m back2future_amd.build --experiments`): using the default%s\n", k.c_str(),
                        c->*r.member, corr ? " kernel" : "", corr ? "" : " (2)");
                c->*r.member = corr ? -1 : 2;
            }
        }
    }
    // a blocking stream: ordered with the legacy default stream like any such stream, so inputs that PyTorch (whose
    // default stream is the null stream) or hipMemcpy / hipMemset produced there are complete before our kernels read them
    if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) {
        delete c;
        return fail("b2f_init: hipStreamCreate failed");
    }
    if (install_weights(c, flat.data(), (long long)flat.size(), past) != 0) {
        b2f_destroy(c);
        return 1;
    }
    *out = c;
    return 0;
}
B2F_CATCH("b2f_init_ex")

void b2f_destroy(b2f_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    while (!c->streams.empty()) b2f_stream_close(c->streams.back());   // the context owns its streams
    drop_graphs(c);
    drop_gen_out(c);
    for (ProfEvent &pe : c->prof_pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (HostSlot &hs : c->slot) {
        if (hs.dev) (void)hipFree(hs.dev);
        if (hs.pin) (void)hipHostFree(hs.pin);
        for (hipEvent_t e : {hs.ev_in, hs.ev_comp, hs.ev_out})
            if (e) (void)hipEventDestroy(e);
    }
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    if (c->dwork.dev) (void)hipFree(c->dwork.dev);
    if (c->vis_max.dev) (void)hipFree(c->vis_max.dev);
    if (c->loss_pyr.dev) (void)hipFree(c->loss_pyr.dev);
    if (c->loss_rec.dev) (void)hipFree(c->loss_rec.dev);
    if (c->loss_work.dev) (void)hipFree(c->loss_work.dev);
    if (c->arena) (void)hipFree(c->arena);
    if (c->wpk_dev) (void)hipFree(c->wpk_dev);
    if (c->w_dev) (void)hipFree(c->w_dev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int b2f_info(const b2f_ctx *c, int *levels, int *win, int *past_flow, int *n_outputs, long long *n_params) try
{
    if (!c) return fail("b2f_info: null context");
    if (levels) *levels = c->g.levels;
    if (win) *win = c->g.win;
    if (past_flow) *past_flow = c->past_flow ? 1 : 0;
    if (n_outputs) *n_outputs = c->g.n_outputs();   // pwc.lua:459-489
    if (n_params) *n_params = c->nparams;
    return 0;
}
B2F_CATCH("b2f_info")

int b2f_set_weights(b2f_ctx *c, const float *host_flat, long long n) try
{
    if (!c || !host_flat) return fail("b2f_set_weights: null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    bool past;
    GraphOpts gp = c->g, gn = c->g;
    gp.past_flow = true; gn.past_flow = false;
    if (n == param_count(gp)) past = true;
    else if (n == param_count(gn)) past = false;
    else return fail("b2f_set_weights: n is neither the Hard nor the Soft parameter count of this graph");
    return install_weights(c, host_flat, n, past);
}
B2F_CATCH("b2f_set_weights")

int b2f_get_weights(b2f_ctx *c, float *host_flat, long long n) try
{
    if (!c || !host_flat || n != c->nparams) return fail("b2f_get_weights: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(host_flat, c->w_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
B2F_CATCH("b2f_get_weights")

int b2f_weights_device(b2f_ctx *c, void **dev_ptr, long long *n) try
{
    if (!c || !dev_ptr) return fail("b2f_weights_device: null argument");
    *dev_ptr = c->w_dev;
    if (n) *n = c->nparams;
    return 0;
}
B2F_CATCH("b2f_weights_device")

int b2f_commit_weights(b2f_ctx *c) try
{
    if (!c) return fail("b2f_commit_weights: null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    drop_graphs(c);   // pack_all may move wpk_dev
    std::vector<float> flat((size_t)c->nparams);
    HIPCHK(hipMemcpy(flat.data(), c->w_dev, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
    return pack_all(c, flat.data());
}
B2F_CATCH("b2f_commit_weights")

int b2f_set_option(b2f_ctx *c, const char *key, int value) try
{
    if (!c || !key) return fail("b2f_set_option: null argument");
    const OptRow *r = find_option(key);
    if (!r) return fail(std::string("b2f_set_option: unknown key ") + key);
    if (!r->member) {
        c->host_subbatch_pixels = value > 0 ? value : (16ll << 20);
        return 0;
    }
    if ((r->flags & OPT_EXP_ONLY) && !B2F_EXPERIMENTS) {
        if (value != 0) return fail(std::string("b2f_set_option: ") + key + " selects an experiment kernel (tools/experiments/csrc): build with `python -m back2future_amd.build --experiments` and load libb2f_exp.so");
        return 0;
    }
    if (r->flags & OPT_SYNC) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipDeviceSynchronize());
        drop_graphs(c);
    }
    if (const char *refusal = experiment_value(*r, value)) return fail(refusal);
    if (r->flags & OPT_ARENA) {
        if (r->member == &b2f_ctx::arena_guard && (value < 0 || value % 64)) return fail("b2f_set_option: arena_guard is a count of floats, a multiple of 64");
        if (r->member == &b2f_ctx::arena_fill && value != 0 && value != 1) return fail("b2f_set_option: arena_fill is 0 or 1");
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipDeviceSynchronize());
        drop_graphs(c);   // the next pass allocates and fills afresh, as after a growth of the arena
        if (c->arena) HIPCHK(hipFree(c->arena));
        c->arena = nullptr;
        c->arena_floats = 0;
        c->guards.clear();
        c->arena_layout[0] = 0;
    }
    const bool had = r->repack && reads_packing(c, r->repack);
    c->*r->member = value;
    if (r->repack && had != reads_packing(c, r->repack)) CHK(b2f_commit_weights(c));
    return 0;
}
B2F_CATCH("b2f_set_option")

int b2f_get_option(const b2f_ctx *c, const char *key, int *value) try
{
    if (!c || !key || !value) return fail("b2f_get_option: null argument");
    const OptRow *r = find_option(key);
    if (!strcmp(key, "experiments")) *value = B2F_EXPERIMENTS;   // read-only: which build this is
    else if (!r) return fail(std::string("b2f_get_option: unknown key ") + key);
    else if (!r->member) *value = (int)std::min<long long>(c->host_subbatch_pixels, 0x7fffffff);
    else *value = c->*r->member;
    return 0;
}
B2F_CATCH("b2f_get_option")

int b2f_synchronize(b2f_ctx *c) try
{
    if (!c) return fail("b2f_synchronize: null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
B2F_CATCH("b2f_synchronize")

int b2f_profile_reset(b2f_ctx *c) try
{
    if (!c) return fail("b2f_profile_reset: null context");
    CHK(prof_collect(c));
    std::fill(c->prof_ms.begin(), c->prof_ms.end(), 0.0);
    std::fill(c->prof_n.begin(), c->prof_n.end(), 0);
    return 0;
}
B2F_CATCH("b2f_profile_reset")

int b2f_profile_read(b2f_ctx *c, char *names, double *total_ms, long long *launches, int cap, int *n) try
{
    if (!c || !n) return fail("b2f_profile_read: null argument");
    CHK(prof_collect(c));
    const int cnt = std::min<int>(cap, (int)c->prof_names.size());
    for (int i = 0; i < cnt; ++i) {
        if (names) { strncpy(names + 32 * i, c->prof_names[i].c_str(), 31); names[32 * i + 31] = 0; }
        if (total_ms) total_ms[i] = c->prof_ms[i];
        if (launches) launches[i] = c->prof_n[i];
    }
    *n = cnt;
    return 0;
}
B2F_CATCH("b2f_profile_read")

}  // extern "C"

// model:forward on device pointers.  With `graph` the ~150 launches of a (shape, pointers) combination are replayed
// from a hipGraph: the first call of a combination runs eagerly (and lets the kernels set their function
// attributes, which must not happen inside a capture), the second one captures, later ones only replay.  Worth
// ~0.5 ms per forward pass: 17 % of a single full-HD triplet, 2 % of a batch of 16.
int b2f::forward_device(b2f_ctx *c, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow, float *dev_occ,
                        float *dev_est3, hipStream_t s, bool graph, bool seq, const StreamPass *sp, float *dev_past)
{
    CHK(check_shape(B, H, W));
    if (dev_past && !c->past_flow)
        return fail("b2f: this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only): there is no past flow to return");
    HIPCHK(hipSetDevice(c->device));
    if (sp && !c->g.shipped()) return fail("b2f_stream_push: streams run on the shipped graph only (this context was made with b2f_init_ex options)");
    if (seq && !c->g.shipped()) return fail("b2f_forward_sequence_device: sequences run on the shipped graph only (this context was made with b2f_init_ex options)");
    if (!c->g.shipped()) {
        // other graph shapes: the whole output table through the generic executor (b2f_graph.hip), then est[1] / the
        // finest occlusion map / est[3] into the caller's buffers.  Asynchronous on the stream like the tuned path, no hipGraph: a correctness path.
        const int n = c->g.n_outputs(), per = c->past_flow ? 5 : 4, lst = c->g.l_st();
        // the output table lives in the context and is re-allocated only when the shape changes (a hipMalloc / hipFree pair per
        // call is device-synchronising and stalled the upload / download overlap of the host pipeline: ADVICE r2)
        if ((int)c->gen_out.size() != n || c->genB != B || c->genH != H || c->genW != W) {
            HIPCHK(hipDeviceSynchronize());
            drop_gen_out(c);
            c->gen_out.assign((size_t)n, nullptr);
            for (int i = 0; i < n; ++i) {
                const int l = lst + i / per, j = i % per;
                const size_t cnt = (size_t)B * (H >> (l - lst)) * (W >> (l - lst)) * ((j >= per - 2) ? 3 : 2);
                if (hipMalloc(&c->gen_out[(size_t)i], cnt * sizeof(float)) != hipSuccess) {
                    drop_gen_out(c);
                    return fail("b2f_forward_device: out of device memory");
                }
            }
            c->genB = B; c->genH = H; c->genW = W;
        }
        std::vector<float *> &dev = c->gen_out;
        CHK(graph_forward(c, s, false, dev_in, in_kind, B, H, W, dev.data()));
        const size_t n2 = (size_t)B * 2 * H * W * sizeof(float);
        if (dev_flow) HIPCHK(hipMemcpyAsync(dev_flow, dev[0], n2, hipMemcpyDeviceToDevice, s));
        if (dev_occ) HIPCHK(hipMemcpyAsync(dev_occ, dev[(size_t)(c->past_flow ? 2 : 1)], n2, hipMemcpyDeviceToDevice, s));
        if (dev_est3) HIPCHK(hipMemcpyAsync(dev_est3, dev[2], c->past_flow ? n2 : n2 / 2 * 3, hipMemcpyDeviceToDevice, s));
        if (dev_past) HIPCHK(hipMemcpyAsync(dev_past, dev[1], n2, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const Plan P = make_plan((size_t)c->arena_guard, B, H, W, false, c->past_flow, seq, sp != nullptr, dev_past != nullptr);
    CHK(ensure_workspace(c, P));
    Outs O;
    O.flow = dev_flow; O.occ = dev_occ; O.est3 = dev_est3; O.past = dev_past;
    if (graph && !c->profile) {
        if (c->graphs.size() > 256) {   // callers that keep changing pointers: start over (replays may still be in flight)
            HIPCHK(hipDeviceSynchronize());
            drop_graphs(c);
        }
        const int req = c->req_batch > 0 ? c->req_batch : B;
        const GraphKey key = {dev_in, dev_flow, dev_occ, dev_est3, in_kind, B, H, W, (c->adaptive_kernels > 0 || (c->adaptive_kernels < 0 && req == 1)) ? 1 : 0,
                              seq ? 1 : 0, sp ? sp->ring : nullptr, sp ? 1 + 2 * sp->slot + (sp->ready ? 1 : 0) : 0, dev_past};
        auto it = c->graphs.find(key);
        if (it == c->graphs.end()) {
            c->graphs.emplace(key, nullptr);
            return forward_impl(c, s, false, dev_in, in_kind, P, O, sp);
        }
        if (!it->second) {
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int rc = forward_impl(c, s, true, dev_in, in_kind, P, O, sp);
            const hipError_t e = hipStreamEndCapture(s, &g);
            if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
            HIPCHK(e);
            hipGraphExec_t ge = nullptr;
            const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            HIPCHK(ei);
            it->second = ge;
        }
        HIPCHK(hipGraphLaunch(it->second, s));
        return 0;
    }
    return forward_impl(c, s, false, dev_in, in_kind, P, O, sp);
}

extern "C" {

int b2f_forward_device(b2f_ctx *c, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow,
                       float *dev_occ, float *dev_est3, void *stream) try
{
    if (!c || !dev_in) return fail("b2f_forward_device: null argument");
    // the glue kernels read / write these planes with 16-byte vector accesses (include/b2f.h states the requirement)
    if (((uintptr_t)dev_in | (uintptr_t)dev_flow | (uintptr_t)dev_occ | (uintptr_t)dev_est3) & 15)
        return fail("b2f_forward_device: device buffers must be 16-byte aligned");
    return forward_device(c, dev_in, in_kind, B, H, W, dev_flow, dev_occ, dev_est3, stream ? (hipStream_t)stream : c->stream,
                          c->use_graph != 0);
}
B2F_CATCH("b2f_forward_device")

int b2f_forward_sequence_device(b2f_ctx *c, const void *dev_frames, int in_kind, int T, int H, int W, float *dev_flow, float *dev_occ,
                                float *dev_est3, void *stream) try
{
    if (!c || !dev_frames) return fail("b2f_forward_sequence_device: null argument");
    if (T < 3) return fail("b2f_forward_sequence_device: a sequence needs T >= 3 frames (one triplet)");
    if (in_kind != B2F_IN_NORMALIZED && in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8)
        return fail("b2f_forward_sequence_device: in_kind must be B2F_IN_NORMALIZED, B2F_IN_UNIT or B2F_IN_U8");
    if (((uintptr_t)dev_frames | (uintptr_t)dev_flow | (uintptr_t)dev_occ | (uintptr_t)dev_est3) & 15)
        return fail("b2f_forward_sequence_device: device buffers must be 16-byte aligned");
    return forward_device(c, dev_frames, in_kind, T - 2, H, W, dev_flow, dev_occ, dev_est3, stream ? (hipStream_t)stream : c->stream,
                          c->use_graph != 0, true);
}
B2F_CATCH("b2f_forward_sequence_device")

int b2f_forward_device_past(b2f_ctx *c, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow, float *dev_past_flow,
                            float *dev_occ, float *dev_est3, void *stream) try
{
    if (!c || !dev_in) return fail("b2f_forward_device_past: null argument");
    if (!c->past_flow)
        return fail("b2f_forward_device_past: this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only)");
    if (((uintptr_t)dev_in | (uintptr_t)dev_flow | (uintptr_t)dev_past_flow | (uintptr_t)dev_occ | (uintptr_t)dev_est3) & 15)
        return fail("b2f_forward_device_past: device buffers must be 16-byte aligned");
    return forward_device(c, dev_in, in_kind, B, H, W, dev_flow, dev_occ, dev_est3, stream ? (hipStream_t)stream : c->stream,
                          c->use_graph != 0, false, nullptr, dev_past_flow);
}
B2F_CATCH("b2f_forward_device_past")

int b2f_forward_sequence_device_past(b2f_ctx *c, const void *dev_frames, int in_kind, int T, int H, int W, float *dev_flow,
                                     float *dev_past_flow, float *dev_occ, float *dev_est3, void *stream) try
{
    if (!c || !dev_frames) return fail("b2f_forward_sequence_device_past: null argument");
    if (!c->past_flow)
        return fail("b2f_forward_sequence_device_past: this model has no past-flow decoders (a Hard or two_frame model estimates the future flow only)");
    if (T < 3) return fail("b2f_forward_sequence_device_past: a sequence needs T >= 3 frames (one triplet)");
    if (in_kind != B2F_IN_NORMALIZED && in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8)
        return fail("b2f_forward_sequence_device_past: in_kind must be B2F_IN_NORMALIZED, B2F_IN_UNIT or B2F_IN_U8");
    if (((uintptr_t)dev_frames | (uintptr_t)dev_flow | (uintptr_t)dev_past_flow | (uintptr_t)dev_occ | (uintptr_t)dev_est3) & 15)
        return fail("b2f_forward_sequence_device_past: device buffers must be 16-byte aligned");
    return forward_device(c, dev_frames, in_kind, T - 2, H, W, dev_flow, dev_occ, dev_est3, stream ? (hipStream_t)stream : c->stream,
                          c->use_graph != 0, true, nullptr, dev_past_flow);
}
B2F_CATCH("b2f_forward_sequence_device_past")

int b2f_output_shapes(const b2f_ctx *c, int H, int W, int *ch, int *oh, int *ow, int cap) try
{
    if (!c) return fail("b2f_output_shapes: null context");
    int no = 0;
    for (int l = c->g.l_st(); l <= c->g.levels; ++l) {
        const int per = c->past_flow ? 5 : 4;
        for (int j = 0; j < per; ++j) {
            if (no >= cap) return fail("b2f_output_shapes: cap too small");
            ch[no] = (j >= per - 2) ? 3 : 2;
            oh[no] = H >> (l - c->g.l_st());
            ow[no] = W >> (l - c->g.l_st());
            ++no;
        }
    }
    return 0;
}
B2F_CATCH("b2f_output_shapes")

int b2f_forward(b2f_ctx *c, const float *x, int B, int H, int W, float **outs, int n_outs) try
{
    if (!c || !x || !outs) return fail("b2f_forward: null argument");
    const bool shipped = c->g.shipped();
    if (shipped) CHK(check_shape(B, H, W));
    else if (B <= 0 || H <= 0 || W <= 0 || H % (1 << (c->g.levels - 1)) || W % (1 << (c->g.levels - 1)))
        return fail("b2f_forward: H and W must be positive multiples of 2^(levels - 1)");
    HIPCHK(hipSetDevice(c->device));
    const int per = c->past_flow ? 5 : 4, lst = c->g.l_st(), lev = c->g.levels;
    if (n_outs != c->g.n_outputs()) return fail("b2f_forward: n_outs must be (levels - skip) x 4 (5 with past-flow decoders): 20 / 25 for the shipped models");
    // arena first (it may be re-allocated), then the per-output device buffers
    Plan P;
    if (shipped) {
        P = make_plan((size_t)c->arena_guard, B, H, W, true, c->past_flow);
        CHK(ensure_workspace(c, P));
    }
    // option arena_guard (tests): every tensor of the table is a guarded device buffer that starts as kGuardWord, checked below
    const bool guarded = c->arena_guard > 0;
    static const char *const kSlot[2][5] = {{"ufs", "occs", "iw1", "iw3", ""}, {"ufs", "ubfs", "occs", "iw1", "iw3"}};
    std::vector<std::string> gname(guarded ? n_outs : 0);
    std::unique_ptr<DevBuf[]> gbuf(guarded ? new DevBuf[n_outs] : nullptr);
    std::vector<float *> dev(n_outs, nullptr);
    std::vector<size_t> cnt(n_outs, 0);
    float *d_in = nullptr;
    int rc = 0;
    auto cleanup = [&]() {
        if (!guarded)
            for (float *p : dev) if (p) (void)hipFree(p);
        if (d_in) (void)hipFree(d_in);
    };
    Outs O;
    int no = 0;
    for (int l = lst; l <= lev && !rc; ++l) {
        const size_t px = (size_t)B * (H >> (l - lst)) * (W >> (l - lst));
        for (int j = 0; j < per; ++j) {
            const int ch = (j >= per - 2) ? 3 : 2;
            cnt[no] = px * ch;
            if (guarded) {
                gname[no] = std::string("b2f_forward output ") + kSlot[c->past_flow ? 1 : 0][j] + "[" + std::to_string(l) + "]";
                if (gbuf[no].alloc(cnt[no], gname[no].c_str())) { rc = 1; break; }
                dev[no] = gbuf[no].p;
            } else if (hipMalloc(&dev[no], cnt[no] * sizeof(float)) != hipSuccess) { rc = fail("b2f_forward: out of device memory"); break; }
            ++no;
        }
        if (rc) break;
        int base = (l - lst) * per, j = 0;
        O.t_ufs[l] = dev[base + j++];
        if (c->past_flow) O.t_ubfs[l] = dev[base + j++];
        O.t_occ[l] = dev[base + j++];
        O.t_iw1[l] = dev[base + j++];
        O.t_iw3[l] = dev[base + j++];
    }
    const size_t nin = (size_t)B * 9 * H * W;
    if (!rc && hipMalloc(&d_in, nin * sizeof(float)) != hipSuccess) rc = fail("b2f_forward: out of device memory");
    if (!rc && hipMemcpyAsync(d_in, x, nin * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail("b2f_forward: H2D copy failed");
    if (!rc) rc = shipped ? forward_impl(c, c->stream, false, d_in, B2F_IN_NORMALIZED, P, O)
                          : graph_forward(c, c->stream, false, d_in, B2F_IN_NORMALIZED, B, H, W, dev.data());
    if (!rc && guarded) {
        if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(std::string("b2f_forward: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n_outs && !rc; ++i) rc = gbuf[i].check();
    }
    for (int i = 0; i < n_outs && !rc; ++i)
        if (hipMemcpyAsync(outs[i], dev[i], cnt[i] * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail("b2f_forward: D2H copy failed");
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(std::string("b2f_forward: ") + hipGetErrorString(hipGetLastError()));
    cleanup();
    return rc;
}
B2F_CATCH("b2f_forward")

}  // extern "C"

// ---- model:forward followed by an objective of the table-loss family (b2f_ctx.h: LossSpec) --------
// Every b2f_forward_loss* entry builds the descriptor of its objective and outputs and calls forward_loss_host or forward_loss_device;
// both cut the request into sub-batches, and forward_loss_run hands each one's table to table_loss_dispatch (b2f_tableloss.hip).
namespace {

// what a b2f_forward_loss* call needs from the context's loss workspace for sub-batches of nb triplets
struct LossPlan {
    int L = 0, per = 0, n_outs = 0;
    int words = B2F_LOSS_WORDS;     // of a record of the objective (LossSpec::words)
    std::vector<size_t> cnt, off;   // floats and byte offset of every tensor of the table
    std::vector<size_t> goff;       // byte offset of every tensor of the gradient table (with_grad)
    size_t in_off = 0, loss_off = 0, bytes = 0;
    size_t gt_off = 0, valid_off = 0, occ_off = 0;   // the ground truth of a sub-batch (kLossEpe from host memory)
};

int check_forward_loss(const b2f_ctx *c, const std::string &w, int n, int H, int W, double flow_scale)
{
    if (c->g.two_frame) return fail(w + ": a two_frame model has no occlusions in its table; the loss of test.lua:266-297 is not defined for it");
    if (c->g.shipped()) CHK(check_shape(n, H, W));
    else if (n <= 0 || H <= 0 || W <= 0 || H % (1 << (c->g.levels - 1)) || W % (1 << (c->g.levels - 1)))
        return fail(w + ": H and W must be positive multiples of 2^(levels - 1)");
    int L = 0;
    const char *why = table_loss_refusal(c->g.n_outputs(), c->past_flow ? 5 : 4, n, H, W, flow_scale, &L);
    if (why) return fail(w + ": " + why);
    return 0;
}

// from_host: the sub-batch's frames, and kLossEpe's ground truth, are uploaded into the workspace; with_grad: so is the gradient table kept there
LossPlan make_loss_plan(const b2f_ctx *c, int nb, int H, int W, const LossSpec &d, bool from_host, bool with_grad)
{
    const bool with_input = from_host, with_truth = from_host && d.is_epe();
    LossPlan p;
    p.words = d.words();
    p.per = c->past_flow ? 5 : 4;
    p.n_outs = c->g.n_outputs();
    p.L = p.n_outs / p.per;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    p.in_off = take(with_input ? (size_t)nb * 9 * H * W * sizeof(float) : 0);
    p.gt_off = take(with_truth ? (size_t)nb * 2 * H * W * sizeof(float) : 0);
    p.valid_off = take(with_truth ? (size_t)nb * H * W : 0);
    p.occ_off = take(with_truth ? (size_t)nb * H * W : 0);
    for (int i = 0; i < p.n_outs; ++i) {
        p.cnt.push_back(table_floats(i, p.per, nb, H, W));
        p.off.push_back(take(p.cnt.back() * sizeof(float)));
    }
    p.loss_off = take((size_t)nb * p.L * p.words * sizeof(unsigned long long));
    if (with_grad)
        for (int i = 0; i < p.n_outs; ++i) p.goff.push_back(take(p.cnt[(size_t)i] * sizeof(float)));
    p.bytes = off;
    return p;
}

// the table of nb triplets into tab (device tensors in table order) on s
int forward_table_run(b2f_ctx *c, hipStream_t s, const float *d_in, int nb, int H, int W, const LossPlan &lp, float *const *tab)
{
    if (c->g.shipped()) {
        const Plan P = make_plan((size_t)c->arena_guard, nb, H, W, true, c->past_flow);
        CHK(ensure_workspace(c, P));
        Outs O;
        for (int j = 0; j < lp.L; ++j) {
            const int l = c->g.l_st() + j;
            int k = j * lp.per;
            O.t_ufs[l] = tab[k++];
            if (c->past_flow) O.t_ubfs[l] = tab[k++];
            O.t_occ[l] = tab[k++];
            O.t_iw1[l] = tab[k++];
            O.t_iw3[l] = tab[k++];
        }
        CHK(forward_impl(c, s, false, d_in, B2F_IN_NORMALIZED, P, O));
    } else {
        CHK(graph_forward(c, s, false, d_in, B2F_IN_NORMALIZED, nb, H, W, tab));
    }
    return 0;
}

// the table of nb triplets into tab, then the objective of the resolved d on it: its records into d_loss and its gradient table into grad,
// each where wanted (else nullptr); all on s.  The reference image is the centre frame; d's ground truth is the device memory of these nb
// triplets.
int forward_loss_run(b2f_ctx *c, hipStream_t s, const float *d_in, int nb, int H, int W, double flow_scale, const LossSpec &d, const LossPlan &lp,
                     float *const *tab, unsigned long long *d_loss, float *const *grad)
{
    CHK(forward_table_run(c, s, d_in, nb, H, W, lp, tab));
    const size_t hw = (size_t)H * W;
    return table_loss_dispatch(c, s, tab, grad, d_loss, d, lp.L, c->past_flow, nb, H, W, d_in + 3 * hw, 9 * hw, flow_scale);
}

// triplets per sub-batch of a b2f_forward_loss* call: the host_subbatch_pixels budget, within the launchers' limit of images
int loss_subbatch(const b2f_ctx *c, int n, int H, int W)
{
    return (int)std::min<long long>(std::min(n, 65535), std::max<long long>(1, c->host_subbatch_pixels / ((long long)H * W)));
}

// what b2f_forward_loss_ssim* check beyond check_forward_loss: the range, and that the batch's range is asked of one sub-batch only (a
// record would depend on where the request is cut otherwise)
int check_forward_loss_kind(const b2f_ctx *c, const std::string &w, const LossSpec &d, int n, int H, int W)
{
    if (!d.ranged()) return 0;
    const char *why = d.range_refusal();
    if (why) return fail(w + ": " + why);
    if (d.range_mode == B2F_SSIM_RANGE_BATCH && loss_subbatch(c, n, H, W) < n)
        return fail(w + ": B2F_SSIM_RANGE_BATCH needs the request in one sub-batch and this one would be cut (host_subbatch_pixels): use "
                        "B2F_SSIM_RANGE_IMAGE or B2F_SSIM_RANGE_GIVEN, which do not depend on the cut");
    return 0;
}

// grows the context's loss workspace to the plan and points tab, and gr where asked (a plan with_grad), at the plan's tensors in it
int loss_work_tables(b2f_ctx *c, const LossPlan &lp, std::vector<float *> &tab, std::vector<float *> *gr)
{
    CHK(ensure_dev_work(c->loss_work, lp.bytes));
    for (int i = 0; i < lp.n_outs; ++i) {
        tab.push_back((float *)(c->loss_work.dev + lp.off[(size_t)i]));
        if (gr) gr->push_back((float *)(c->loss_work.dev + lp.goff[(size_t)i]));
    }
    return 0;
}

// what the b2f_forward_loss_grad* and b2f_forward_loss_epe* entries check beyond check_forward_loss: d.resolve -- the supervised objective
// in front of the gradient table's pointers, the others behind them --, and those pointers where there is a gradient table
int check_forward_loss_grad(const b2f_ctx *c, const std::string &w, LossSpec &d, float *const *grad, int n_outs)
{
    const char *why = d.is_epe() ? d.resolve(c->g.n_outputs() / (c->past_flow ? 5 : 4)) : nullptr;
    if (why) return fail(w + ": " + why);
    if (grad && n_outs != c->g.n_outputs()) return fail(w + ": n_outs must be (levels - skip) x 4 (5 with past-flow decoders): 20 / 25 for the shipped models");
    for (int i = 0; grad && i < n_outs; ++i) {
        if (!grad[i]) return fail(w + ": null tensor in the gradient table");
        if (d.is_epe() && ((const void *)grad[i] == (const void *)d.gt_flow || (const void *)grad[i] == (const void *)d.valid || (const void *)grad[i] == (const void *)d.gt_occ))
            return fail(w + ": the gradient table must not alias the ground truth");
        for (int k = 0; k < i; ++k)
            if (grad[i] == grad[k]) return fail(w + ": the gradient table must not alias itself");
    }
    if (!d.is_epe() && (why = d.resolve(0))) return fail(w + ": " + why);
    return 0;
}

// kLossEpe from host memory with size_average, a gradient table and the batch's counts, on a request that is cut: N_j, N'_j over the
// caller's whole n first, into `whole`, and given to every sub-batch -- the cut changes nothing
void whole_request_counts(const b2f_ctx *c, LossSpec &d, bool with_grad, int n, int H, int W, std::vector<double> &whole)
{
    if (!d.is_epe() || !with_grad || !d.epe.size_average || d.count_mode != B2F_EPE_COUNT_BATCH || loss_subbatch(c, n, H, W) >= n) return;
    const int L = c->g.n_outputs() / (c->past_flow ? 5 : 4);
    std::vector<unsigned long long> cnt((size_t)n * L * 2);
    epe_counts_host(d.valid, d.epe.occ > 0.0 ? d.gt_occ : nullptr, L, n, H, W, cnt.data());
    whole.assign((size_t)L * 2, 0.0);
    for (int j = 0; j < 2 * L; ++j) {
        unsigned long long all = 0;
        for (int b = 0; b < n; ++b) all += cnt[(size_t)b * L * 2 + j];
        whole[(size_t)j] = (double)all;
    }
    d.count_mode = B2F_EPE_COUNT_GIVEN;
    d.counts = whole.data();
}

struct ReqBatchScope {   // the kernel rule follows the caller's n while its sub-batches run (b2f_ctx::req_batch)
    b2f_ctx *c;
    ReqBatchScope(b2f_ctx *cc, int n) : c(cc) { c->req_batch = n; }
    ~ReqBatchScope() { c->req_batch = 0; }
};

// the sub-batch loop of the b2f_forward_loss* entries of every objective on checked arguments: upload, forward_loss_run, download of the
// records (loss), the gradient table (grad) and the table (outs), each where not null.  kLossEpe: the host ground truth of the n triplets
// is uploaded with the frames of each sub-batch.
int forward_loss_host_run(b2f_ctx *c, const float *x, int n, int req, int H, int W, double flow_scale, const LossSpec &d, unsigned long long *loss,
                          float *const *grad, float *const *outs)
{
    HIPCHK(hipSetDevice(c->device));
    const size_t hw = (size_t)H * W;
    const int sb = loss_subbatch(c, n, H, W);
    const LossPlan lp = make_loss_plan(c, sb, H, W, d, true, grad != nullptr);
    std::vector<float *> tab, gr;
    CHK(loss_work_tables(c, lp, tab, grad ? &gr : nullptr));
    float *d_in = (float *)(c->loss_work.dev + lp.in_off);
    unsigned long long *d_loss = loss ? (unsigned long long *)(c->loss_work.dev + lp.loss_off) : nullptr;
    ReqBatchScope rb(c, req > 0 ? req : n);
    hipStream_t s = c->stream;
    for (int b0 = 0; b0 < n; b0 += sb) {
        const int nb = std::min(sb, n - b0);
        HIPCHK(hipMemcpyAsync(d_in, x + (size_t)b0 * 9 * hw, (size_t)nb * 9 * hw * sizeof(float), hipMemcpyHostToDevice, s));
        LossSpec dd = d;
        if (d.is_epe()) {   // the sub-batch's ground truth, behind its frames on the same stream
            const LossSpec h = d.at_image((size_t)b0, hw);
            float *d_gt = (float *)(c->loss_work.dev + lp.gt_off);
            unsigned char *d_valid = (unsigned char *)(c->loss_work.dev + lp.valid_off), *d_occ = (unsigned char *)(c->loss_work.dev + lp.occ_off);
            HIPCHK(hipMemcpyAsync(d_gt, h.gt_flow, (size_t)nb * 2 * hw * sizeof(float), hipMemcpyHostToDevice, s));
            if (h.valid) HIPCHK(hipMemcpyAsync(d_valid, h.valid, (size_t)nb * hw, hipMemcpyHostToDevice, s));
            if (h.gt_occ) HIPCHK(hipMemcpyAsync(d_occ, h.gt_occ, (size_t)nb * hw, hipMemcpyHostToDevice, s));
            dd.gt_flow = d_gt;
            dd.valid = h.valid ? d_valid : nullptr;
            dd.gt_occ = h.gt_occ ? d_occ : nullptr;
        }
        // (a shorter last sub-batch lays its tensors out for nb images in the same buffers)
        CHK(forward_loss_run(c, s, d_in, nb, H, W, flow_scale, dd, lp, tab.data(), d_loss, grad ? gr.data() : nullptr));
        if (loss)
            HIPCHK(hipMemcpyAsync(loss + (size_t)b0 * lp.L * lp.words, d_loss, (size_t)nb * lp.L * lp.words * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, s));
        for (int i = 0; i < lp.n_outs; ++i) {
            const size_t per_img = lp.cnt[(size_t)i] / (size_t)sb;
            if (grad) HIPCHK(hipMemcpyAsync(grad[i] + (size_t)b0 * per_img, gr[(size_t)i], (size_t)nb * per_img * sizeof(float), hipMemcpyDeviceToHost, s));
            if (outs) HIPCHK(hipMemcpyAsync(outs[i] + (size_t)b0 * per_img, tab[(size_t)i], (size_t)nb * per_img * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}

}  // namespace

// the b2f_forward_loss* entries of every objective from host memory, and a shard of theirs: `req` is the caller's n
int b2f::forward_loss_host(b2f_ctx *c, const float *x, int n, int req, int H, int W, double flow_scale, LossSpec d, unsigned long long *loss, float *const *grad,
                           int n_outs, float *const *outs)
{
    const std::string w = std::string("b2f_forward_loss") + d.suffix();
    const char *why = !c || !x ? "null argument" : d.outputs_refusal(loss, grad);
    if (why) return fail(w + ": " + why);
    CHK(check_forward_loss(c, w, n, H, W, flow_scale));
    CHK(check_forward_loss_kind(c, w, d, n, H, W));
    if (!d.is_epe() && !d.grad_entry) {   // the records alone: the table is downloaded with n_outs, or not at all
        if ((outs == nullptr) != (n_outs == 0)) return fail(w + ": outs and n_outs go together (NULL and 0: the table is not downloaded)");
        if (outs && n_outs != c->g.n_outputs()) return fail(w + ": n_outs must be 0 or (levels - skip) x 4 (5 with past-flow decoders): 20 / 25 for the shipped models");
        for (int i = 0; i < n_outs; ++i)
            if (!outs[i]) return fail(w + ": null tensor in outs");
    } else {
        CHK(check_forward_loss_grad(c, w, d, grad, n_outs));
        if (!grad && outs && n_outs != c->g.n_outputs()) return fail(w + ": n_outs must be (levels - skip) x 4 (5 with past-flow decoders): 20 / 25 for the shipped models");
        for (int i = 0; outs && i < n_outs; ++i) {
            if (!outs[i]) return fail(w + ": null tensor in outs");
            for (int k = 0; grad && k < n_outs; ++k)
                if (outs[i] == grad[k]) return fail(w + ": the gradient table must not alias outs");
        }
    }
    std::vector<double> whole;
    whole_request_counts(c, d, grad != nullptr, n, H, W, whole);
    return forward_loss_host_run(c, x, n, req, H, W, flow_scale, d, loss, grad, outs);
}

extern "C" {

// model:forward + the gradient table of train.lua:428-468 from host memory
int b2f_forward_loss_grad(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_opts *opts, unsigned long long *loss,
                          float *const *grad, int n_outs, float *const *outs) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_grad(opts), loss, grad, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_grad")

// the same with the fine-tuning criteria of README.md:89-102 and the 24-word records
int b2f_forward_loss_grad_ft(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_ft_opts *opts,
                             unsigned long long *loss, float *const *grad, int n_outs, float *const *outs) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_grad(opts), loss, grad, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_grad_ft")

extern "C++" {
// every b2f_forward_loss*_device entry; d's ground truth is the device memory of the n triplets
static int forward_loss_device(const std::string &w, b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, LossSpec d,
                               unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream)
{
    if (!c || !dev_in || d.outputs_refusal(dev_loss, dev_grad)) return fail(w + ": null argument");
    if (in_kind != B2F_IN_NORMALIZED) return fail(w + ": in_kind must be B2F_IN_NORMALIZED (the reference image of the loss is the normalized centre frame)");
    CHK(check_forward_loss(c, w, n, H, W, flow_scale));
    CHK(check_forward_loss_kind(c, w, d, n, H, W));
    const int sb = loss_subbatch(c, n, H, W);
    if (d.is_epe() || d.grad_entry) CHK(check_forward_loss_grad(c, w, d, dev_grad, n_outs));
    // (the host entry counts over the whole request instead: whole_request_counts)
    if (d.is_epe() && dev_grad && d.epe.size_average && d.count_mode == B2F_EPE_COUNT_BATCH && sb < n)
        return fail(w + ": B2F_EPE_COUNT_BATCH needs the request in one sub-batch and this one would be cut (host_subbatch_pixels): use "
                        "B2F_EPE_COUNT_IMAGE or B2F_EPE_COUNT_GIVEN, which do not depend on the cut");
    uintptr_t bits = (uintptr_t)dev_in | (uintptr_t)dev_loss | (uintptr_t)d.gt_flow;
    for (int i = 0; dev_grad && i < n_outs; ++i) bits |= (uintptr_t)dev_grad[i];
    if (bits & 15) return fail(w + ": device buffers must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    const size_t hw = (size_t)H * W;
    const LossPlan lp = make_loss_plan(c, sb, H, W, d, false, false);
    std::vector<float *> tab, gr((size_t)lp.n_outs);
    CHK(loss_work_tables(c, lp, tab, nullptr));
    ReqBatchScope rb(c, n);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int b0 = 0; b0 < n; b0 += sb) {
        // the sub-batch's part of the caller's gradient tensors, and of the ground truth: image b0 of every one
        for (int i = 0; dev_grad && i < lp.n_outs; ++i) gr[(size_t)i] = dev_grad[i] + (size_t)b0 * (lp.cnt[(size_t)i] / (size_t)sb);
        CHK(forward_loss_run(c, s, (const float *)dev_in + (size_t)b0 * 9 * hw, std::min(sb, n - b0), H, W, flow_scale, d.at_image((size_t)b0, hw), lp, tab.data(),
                             dev_loss ? dev_loss + (size_t)b0 * lp.L * lp.words : nullptr, dev_grad ? gr.data() : nullptr));
    }
    return 0;
}
}  // extern "C++"

// model:forward + the supervised objective of train.lua:296-334 (criterions/L2Criterion.lua:27-71) from host memory
int b2f_forward_loss_epe(b2f_ctx *c, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                         double flow_scale, const b2f_loss_epe_opts *opts, int count_mode, const double *counts, unsigned long long *loss,
                         float *const *grad, int n_outs, float *const *outs) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_epe(gt_flow, valid, gt_occ, opts, count_mode, counts), loss, grad, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_epe")

// the same on device pointers
int b2f_forward_loss_epe_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, const float *dev_gt_flow,
                                const unsigned char *dev_valid, const unsigned char *dev_gt_occ, double flow_scale, const b2f_loss_epe_opts *opts,
                                int count_mode, const double *counts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_epe(dev_gt_flow, dev_valid, dev_gt_occ, opts, count_mode, counts), dev_loss,
                               dev_grad, n_outs, stream);
}
B2F_CATCH("b2f_forward_loss_epe_device")

// model:forward + the gradient table of train.lua:428-468 on device pointers
int b2f_forward_loss_grad_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, const b2f_loss_grad_opts *opts,
                                 unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_grad(opts), dev_loss, dev_grad, n_outs, stream);
}
B2F_CATCH("b2f_forward_loss_grad_device")

int b2f_forward_loss_grad_ft_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                    const b2f_loss_grad_ft_opts *opts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_grad(opts), dev_loss, dev_grad, n_outs, stream);
}
B2F_CATCH("b2f_forward_loss_grad_ft_device")

// model:forward + the gradient table with the SSIM + L1 photometric term and the 32-word records, from host memory
int b2f_forward_loss_grad_ssim(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_ssim_opts *opts,
                               unsigned long long *loss, float *const *grad, int n_outs, float *const *outs, int range_mode, const float *ranges) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_grad(opts, range_mode, ranges), loss, grad, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_grad_ssim")

int b2f_forward_loss_grad_ssim_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                      const b2f_loss_grad_ssim_opts *opts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream,
                                      int range_mode, const float *ranges) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_grad(opts, range_mode, ranges), dev_loss, dev_grad, n_outs, stream);
}
B2F_CATCH("b2f_forward_loss_grad_ssim_device")

// model:forward + the gradient table with the photometric terms without occlusion masking and the 40-word records, from host memory
int b2f_forward_loss_grad_plain(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_plain_opts *opts,
                                unsigned long long *loss, float *const *grad, int n_outs, float *const *outs, int range_mode, const float *ranges) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_grad(opts, range_mode, ranges), loss, grad, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_grad_plain")

int b2f_forward_loss_grad_plain_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                       const b2f_loss_grad_plain_opts *opts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs, void *stream,
                                       int range_mode, const float *ranges) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_grad(opts, range_mode, ranges), dev_loss, dev_grad, n_outs, stream);
}
B2F_CATCH("b2f_forward_loss_grad_plain_device")

// model:forward + test.lua:266-297 + the photometric sums of criterions/MBCCriterion.lua:35-102 and MSSIML1Criterion.lua:45-153 from
// host memory: loss n x L x 40 words
int b2f_forward_loss_plain(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, float **outs, int n_outs,
                           int range_mode, const float *ranges) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_records(kLossPlain, range_mode, ranges), loss, nullptr, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_plain")

// ... on device pointers: dev_loss n x L x 40 words
int b2f_forward_loss_plain_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, unsigned long long *dev_loss,
                                  void *stream, int range_mode, const float *ranges) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_records(kLossPlain, range_mode, ranges), dev_loss, nullptr, 0, stream);
}
B2F_CATCH("b2f_forward_loss_plain_device")

// model:forward + test.lua:266-297 from host memory
int b2f_forward_loss(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, float **outs, int n_outs) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_records(kLossPme), loss, nullptr, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss")

// model:forward + test.lua:266-297 + the fine-tuning terms of README.md:89-102 from host memory
int b2f_forward_loss_ft(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, float **outs, int n_outs) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_records(kLossFt), loss, nullptr, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_ft")

// model:forward + test.lua:266-297 on device pointers
int b2f_forward_loss_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, unsigned long long *dev_loss,
                            void *stream) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_records(kLossPme), dev_loss, nullptr, 0, stream);
}
B2F_CATCH("b2f_forward_loss_device")

// ... with the fine-tuning terms of README.md:89-102: dev_loss n x L x 24 words
int b2f_forward_loss_ft_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, unsigned long long *dev_loss,
                               void *stream) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_records(kLossFt), dev_loss, nullptr, 0, stream);
}
B2F_CATCH("b2f_forward_loss_ft_device")

// model:forward + test.lua:266-297 + the SSIM + L1 sums of criterions/OSSIML1Criterion.lua:47-163 from host memory: loss n x L x 32 words
int b2f_forward_loss_ssim(b2f_ctx *c, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, float **outs, int n_outs,
                          int range_mode, const float *ranges) try
{
    return forward_loss_host(c, x, n, 0, H, W, flow_scale, loss_records(kLossSsim, range_mode, ranges), loss, nullptr, n_outs, outs);
}
B2F_CATCH("b2f_forward_loss_ssim")

// ... on device pointers: dev_loss n x L x 32 words
int b2f_forward_loss_ssim_device(b2f_ctx *c, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale, unsigned long long *dev_loss,
                                 void *stream, int range_mode, const float *ranges) try
{
    return forward_loss_device(__func__, c, dev_in, in_kind, n, H, W, flow_scale, loss_records(kLossSsim, range_mode, ranges), dev_loss, nullptr, 0, stream);
}
B2F_CATCH("b2f_forward_loss_ssim_device")

}  // extern "C"

extern "C" {

// ---- guards (tests) -------------------------------------------------------------

// The guards of the plan the arena was last filled for: how many of their words no longer hold what the arena was filled with (kGuardWord
// with arena_fill = 1, else 0), compared on bits.  *buffer_index / *offset: the first such word -- the plan's buffer it belongs to and its
// offset from that buffer's end (>= 0: behind the buffer) or from its start (< 0: the guard in front of buffer 0).  b2f_last_error names
// the buffer.  0 without arena_guard; -1 on an error.
int b2f_arena_check(b2f_ctx *c, int *buffer_index, long long *offset) try
{
    if (buffer_index) *buffer_index = -1;
    if (offset) *offset = 0;
    if (!c) { fail("b2f_arena_check: null context"); return -1; }
    if (!c->arena_guard || !c->arena || c->guards.empty()) return 0;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { fail(std::string("b2f_arena_check: ") + hipGetErrorString(hipGetLastError())); return -1; }
    const uint32_t want = c->arena_fill ? kGuardWord : 0u;
    long long bad = 0;
    std::vector<uint32_t> host;
    for (const ArenaGuard &g : c->guards) {
        host.resize(g.len);
        if (g.off + g.len > c->arena_floats) { fail("b2f_arena_check: a guard lies outside the arena"); return -1; }
        if (hipMemcpy(host.data(), c->arena + g.off, g.len * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fail("b2f_arena_check: hipMemcpy failed"); return -1; }
        for (size_t i = 0; i < g.len; ++i) {
            if (host[i] == want) continue;
            if (!bad++) {
                const long long o = g.before ? (long long)i - (long long)g.len : (long long)i;
                if (buffer_index) *buffer_index = g.buffer;
                if (offset) *offset = o;
                char msg[200];
                snprintf(msg, sizeof msg, "arena guard overwritten: the first word %s buffer '%s' (buffer %d of the plan) at offset %+lld from its %s holds 0x%08x",
                         g.before ? "before" : "after", g.name, g.buffer, o, g.before ? "start" : "end", host[i]);
                fail(msg);
            }
        }
    }
    return (int)std::min<long long>(bad, 0x7fffffff);
}
catch (const std::exception &e) { fail(std::string("b2f_arena_check: ") + e.what()); return -1; }
catch (...) { fail("b2f_arena_check: unknown exception"); return -1; }

// Proof that the two detectors detect.  One guard word is overwritten by a hipMemcpy from the host (no kernel stores out of range):
// which = 0: offset +3 behind buffer 1 of the arena's current plan; 1: offset -2 in front of its buffer 0 (b2f_arena_check then reports
// exactly that; needs arena_guard and a pass that has laid the arena out); 2 / 3: offset +2 behind / -1 in front of a guarded device
// buffer 'selftest' of the op-level entries, whose check then fails this call with the buffer's name; 4 / 5: offset +2 behind buffer 'b' /
// -1 in front of buffer 'c' of an OpStage that holds 'a' (10 floats, uploaded), 'b' (1000 floats) and 'c' (7 bytes, uploaded): its finish()
// fails in the same words, though nobody handed it a list of its buffers.
int b2f_guard_selftest(b2f_ctx *c, int which) try
{
    if (!c) return fail("b2f_guard_selftest: null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    const uint32_t word = 0x3f800000u;
    if (which == 0 || which == 1) {
        if (!c->arena_guard || !c->arena || c->guards.size() < 3) return fail("b2f_guard_selftest: no guarded plan (set arena_guard and run a pass first)");
        const ArenaGuard &g = c->guards[which == 0 ? 2 : 0];   // guards[0]: before buffer 0; guards[1 + i]: after buffer i
        const size_t at = which == 0 ? g.off + 3 : g.off + g.len - 2;
        HIPCHK(hipMemcpy(c->arena + at, &word, sizeof word, hipMemcpyHostToDevice));
        return 0;
    }
    if (which == 2 || which == 3) {
        DevBuf b;
        CHK(b.alloc(1000, "selftest"));
        HIPCHK(hipMemcpy(which == 2 ? b.p + b.n + 2 : b.p - 1, &word, sizeof word, hipMemcpyHostToDevice));
        return b.check();
    }
    if (which == 4 || which == 5) {
        const float a10[10] = {0.f};
        const unsigned char c7[7] = {0};
        float *a, *b;
        unsigned char *cc;
        OpStage st(c, __func__);
        CHK(st.in(a10, 10, "a", &a)); CHK(st.out(1000, "b", &b)); CHK(st.in(c7, 7, "c", &cc));
        HIPCHK(hipMemcpy(which == 4 ? b + 1000 + 2 : (float *)cc - 1, &word, sizeof word, hipMemcpyHostToDevice));
        return st.finish();
    }
    return fail("b2f_guard_selftest: which must be 0 .. 5");
}
B2F_CATCH("b2f_guard_selftest")

// make_plan without a context or a device: the float offset of every buffer of the arena, in the order img, tmp, cs[2..7], U[3..6],
// UB[3..6], cv, d[1..5], fs, bfs, logits, u2, flow_planar, ds[2..5] (33 values; 0 for a buffer the plan does not hold), and the total.
// flags: 1 full table, 2 Soft model, 4 sequence, 8 stream push, 16 past-flow output.  Returns 33, or -1.
int b2f_arena_plan(int arena_guard, int B, int H, int W, int flags, long long *offsets, int cap, long long *total) try
{
    if (!offsets || cap < 33 || arena_guard < 0 || arena_guard % 64) { fail("b2f_arena_plan: bad argument"); return -1; }
    if (check_shape(B, H, W)) return -1;
    const Plan p = make_plan((size_t)arena_guard, B, H, W, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0, (flags & 16) != 0);
    int n = 0;
    offsets[n++] = (long long)p.img;
    offsets[n++] = (long long)p.tmp;
    for (int l = 2; l <= 7; ++l) offsets[n++] = (long long)p.cs[l];
    for (int l = 3; l <= 6; ++l) offsets[n++] = (long long)p.U[l];
    for (int l = 3; l <= 6; ++l) offsets[n++] = (long long)p.UB[l];
    offsets[n++] = (long long)p.cv;
    for (int i = 1; i <= 5; ++i) offsets[n++] = (long long)p.d[i];
    for (size_t o : {p.fs, p.bfs, p.logits, p.u2, p.flow_planar}) offsets[n++] = (long long)o;
    for (int k = 2; k <= 5; ++k) offsets[n++] = (long long)p.ds[k];
    if (total) *total = (long long)p.total;
    return n;
}
catch (const std::exception &e) { fail(std::string("b2f_arena_plan: ") + e.what()); return -1; }
catch (...) { fail("b2f_arena_plan: unknown exception"); return -1; }

}  // extern "C"

// ---- what kind of memory a caller's pointer is: the one place that asks the runtime ----
int b2f::pointer_kind(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeArray) return -1;
    return a.type == hipMemoryTypeHost ? 1 : 0;
}

int b2f::check_device_pointers(const std::string &w, const b2f_ctx *c, const char *use, const void *const *ptrs, size_t count, size_t aligned)
{
    uintptr_t bits = 0;
    for (size_t i = 0; i < aligned; ++i) bits |= (uintptr_t)ptrs[i];
    if (bits & 15) return fail(w + ": device buffers must be 16-byte aligned");
    if (!c) return fail(w + ": null context");
    HIPCHK(hipSetDevice(c->device));
    for (size_t i = 0; i < count; ++i)
        if (ptrs[i] && host_memory(ptrs[i])) return fail(w + ": host memory passed to a device entry point (use " + use + ")");
    return 0;
}

// The profile bracket for launches outside this file (the score stage of b2f_pipeline.hip): with profile = 1, a row `name` of
// b2f_profile_read timed by HIP events on the launch stream, like the rows of the forward pass
bool b2f::prof_open(b2f_ctx *c, hipStream_t s, const char *name, ProfEvent *pe)
{
    if (!c->profile) return false;
    pe->name = prof_id(c, name);
    pe->a = get_event(c);
    pe->b = get_event(c);
    (void)hipEventRecord(pe->a, s);
    return true;
}

void b2f::prof_close(b2f_ctx *c, hipStream_t s, const ProfEvent &pe)
{
    (void)hipEventRecord(pe.b, s);
    c->prof_pending.push_back(pe);
}
