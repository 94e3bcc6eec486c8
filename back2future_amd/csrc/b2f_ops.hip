// The kernel test entries of libb2f.so (include/b2f.h: b2f_op_*): host pointers in the reference modules' or the kernels' own layouts, one
// launcher per entry.  Every device buffer of an entry belongs to an OpStage (b2f_ctx.h): guarded on both sides, kGuardWord inside until
// something writes it, and checked by finish() once the stream has been synchronised.  The entries of kernels that are local to another
// file live there (b2f_graph.hip, b2f_backward.hip, b2f_vis.hip, b2f_score.hip, b2f_warp.hip, b2f_tableloss.hip) and use the same scope.
#include "b2f_ctx.h"

#include <cstdio>

using namespace b2f;

namespace b2f {

int DevBuf::alloc(size_t count, const char *what)
{
    n = std::max<size_t>(count, 1);
    name = what;
    const size_t all = n + 2 * kGuardFloats;
    HIPCHK(hipMalloc(&raw, all * sizeof(float)));
    p = raw + kGuardFloats;   // hipMalloc aligns to 256 bytes and the guard is a multiple of that
    HIPCHK(hipMemsetD32((hipDeviceptr_t)raw, (int)kGuardWord, all));
    HIPCHK(hipStreamSynchronize(nullptr));   // the fill is asynchronous on the null stream
    return 0;
}

int DevBuf::check() const
{
    if (!raw) return 0;
    std::vector<uint32_t> g(2 * kGuardFloats);
    HIPCHK(hipMemcpy(g.data(), raw, kGuardFloats * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g.data() + kGuardFloats, p + n, kGuardFloats * sizeof(float), hipMemcpyDeviceToHost));
    long long first = 0, bad = 0;
    bool before = false;
    for (size_t i = 0; i < g.size(); ++i) {
        if (g[i] == kGuardWord) continue;
        if (!bad++) { before = i < kGuardFloats; first = before ? (long long)i - (long long)kGuardFloats : (long long)(i - kGuardFloats); }
    }
    if (!bad) return 0;
    char msg[256];
    snprintf(msg, sizeof msg, "guard of device buffer '%s' (%zu floats) overwritten: %lld words, the first one %s the buffer at offset %+lld from its %s",
             name, n, bad, before ? "before" : "after", first, before ? "start" : "end");
    return api_fail(msg);
}

int OpStage::begin(bool args_ok, const char *what)
{
    if (!c_ || !args_ok) return api_fail(fn_ + ": " + what);
    HIPCHK(hipSetDevice(c_->device));
    return 0;
}

int OpStage::stage(const void *host, size_t bytes, const char *name, void **dev)
{
    DevBuf &d = bufs_.emplace_back();
    CHK(d.alloc((bytes + 3) / 4, name));
    if (host) HIPCHK(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice));
    *dev = d.p;
    return 0;
}

int OpStage::finish()
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c_->stream));
    for (const DevBuf &d : bufs_) CHK(d.check());
    finished_ = true;
    return 0;
}

int OpStage::download(void *host, const void *dev, size_t bytes) const
{
    if (!finished_) return api_fail(fn_ + ": download before the guards were checked");
    HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

void pack_first_conv(const float *w, float *wp)
{
    for (int o = 0; o < 16; ++o)
        for (int t = 0; t < 27; ++t) wp[(size_t)t * 16 + o] = w[(size_t)o * 27 + t];
}

}  // namespace b2f

static int fail(const std::string &m) { return api_fail(m); }

// ---- host layout loops ----------------------------------------------------------------------

// chunk-planar [image][(C + 7) / 8][hw][8] -> planar [image][C][hw]
static void cp8_to_planar(const float *src, size_t images, int C, size_t hw, float *dst)
{
    const size_t Cp = (size_t)(C + 7) / 8 * 8;
    for (size_t n = 0; n < images; ++n)
        for (int ch = 0; ch < C; ++ch) {
            const float *s = src + (n * Cp + (size_t)(ch / 8) * 8) * hw + (ch & 7);
            float *d = dst + (n * C + ch) * hw;
            for (size_t i = 0; i < hw; ++i) d[i] = s[i * 8];
        }
}

// planar [image][Cin][hw] -> chunk-planar [image][C / 8][hw][8], C a multiple of 8.  map (nullptr: the identity, C = Cin): the planar
// channel that chunk-planar channel k holds, or -1 for a hole, which is filled with hole + k / 256.
static void planar_to_cp8(const float *src, size_t images, int Cin, size_t hw, const int *map, float hole, int C, float *dst)
{
    for (size_t n = 0; n < images; ++n)
        for (int k = 0; k < C; ++k) {
            const int ci = map ? map[k] : k;
            const float fill = hole + (float)k / 256.0f;
            const float *s = ci >= 0 ? src + (n * Cin + ci) * hw : nullptr;
            float *d = dst + (n * C + (size_t)(k / 8) * 8) * hw + (k & 7);
            for (size_t i = 0; i < hw; ++i) d[i * 8] = s ? s[i] : fill;
        }
}

// The shape, stride and option fields of the CorrLaunch of b2f_op_warp_costvol (layout 0: NHWC strides, C a multiple of 8 after padding) and
// of b2f_op_cv_record (layout 1: the forward's chunk-planar strides, option corr_ablate); b2f_op_cv_variant asks the launcher's rule about the
// same structure, so what it reports is what those two run.  Pointers and k are left to the caller.
static CorrLaunch op_corr_launch(const b2f_ctx *c, int layout, int B, int C, int h, int w)
{
    const size_t hw = (size_t)h * w;
    CorrLaunch cl{};
    cl.img_stride = (long)(hw * C);
    cl.out_img_stride = (long)(hw * kCvRec);
    if (layout == 0) {   // NHWC expressed with strides
        cl.chunk_stride = 8; cl.pix_stride = C;
        cl.out_chunk_stride = 8; cl.out_pix_stride = kCvRec;
    } else {
        cl.chunk_stride = (long)(hw * 8); cl.pix_stride = 8;
        cl.out_chunk_stride = (long)(hw * 8); cl.out_pix_stride = 8;
        cl.ablate = c->corr_ablate;
    }
    cl.B = B; cl.C = C; cl.h = h; cl.w = w;
    cl.variant = c->corr_variant;
    return cl;
}

extern "C" {

// ---- reference module layouts ------------------------------------------------------------------

int b2f_op_warp_bhwd(b2f_ctx *c, const float *img, const float *grid, int B, int ih, int iw, int C, int gh,
                     int gw, float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(img && grid && out));
    const size_t ni = (size_t)B * ih * iw * C, ng = (size_t)B * gh * gw * 2, no = (size_t)B * gh * gw * C;
    float *di, *dg, *dout;
    CHK(st.in(img, ni, "img", &di)); CHK(st.in(grid, ng, "grid", &dg)); CHK(st.out(no, "out", &dout));
    HIPCHK(launch_warp_nhwc(di, (long)((size_t)ih * iw * C), C, C, ih, iw, dg, 1.0f, B, gh, gw, dout, C, c->stream));
    CHK(st.finish());
    return st.get(out, dout, no);
}
B2F_CATCH("b2f_op_warp_bhwd")

int b2f_op_image_scale(b2f_ctx *c, const float *src, int C, int Hs, int Ws, int normalize, float *dst, int Hd, int Wd) try
{
    OpStage st(c, __func__);
    CHK(st.begin(src && dst));
    if (C <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return fail("b2f_op_image_scale: bad shape");
    const size_t ns = (size_t)C * Hs * Ws, nt = (size_t)C * Hs * Wd, nd = (size_t)C * Hd * Wd;
    float *ds, *dt, *dd;
    CHK(st.in(src, ns, "src", &ds)); CHK(st.out(nt, "row pass", &dt)); CHK(st.out(nd, "dst", &dd));
    HIPCHK(launch_image_scale(ds, normalize, C, Hs, Ws, dt, dd, Hd, Wd, c->stream));
    CHK(st.finish());
    return st.get(dst, dd, nd);
}
B2F_CATCH("b2f_op_image_scale")

int b2f_op_upsample_flow2x(b2f_ctx *c, const float *x, int B, int h, int w, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && y));
    const size_t n = (size_t)B * 2 * h * w;
    float *dp, *dn, *dy;
    CHK(st.in(x, n, "x planar", &dp)); CHK(st.out(n, "x", &dn)); CHK(st.out(4 * n, "y", &dy));
    HIPCHK(launch_planar_to_nhwc(dp, 2, B, h, w, dn, 2, c->stream));
    HIPCHK(launch_upsample_flow2x_planar(dn, 2, B, h, w, dy, c->stream));
    CHK(st.finish());
    return st.get(y, dy, 4 * n);
}
B2F_CATCH("b2f_op_upsample_flow2x")

int b2f_op_warp_costvol(b2f_ctx *c, const float *ref, const float *nbr_future, const float *nbr_past,
                        const float *flow, float k, int B, int C, int h, int w, float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(ref && nbr_future && nbr_past && out));
    const int Cp = (C + 7) / 8 * 8;   // the fused kernel walks channels in chunks of 8; zero channels add 0
    const size_t hw = (size_t)h * w, nplanar = (size_t)B * C * hw, nn = (size_t)B * hw * Cp, nfl = (size_t)B * 2 * hw;
    float *dpl, *dsts[3], *dcv, *dfl_pl, *dfl = nullptr;
    CHK(st.out(nplanar, "planar staging", &dpl)); CHK(st.out(nn, "ref", &dsts[0])); CHK(st.out(nn, "nbr_future", &dsts[1]));
    CHK(st.out(nn, "nbr_past", &dsts[2])); CHK(st.out((size_t)B * hw * kCvRec, "record", &dcv));
    const float *srcs[3] = {ref, nbr_future, nbr_past};
    for (int i = 0; i < 3; ++i) {   // one staging buffer: the stream is drained before the next upload overwrites it
        HIPCHK(hipMemcpyAsync(dpl, srcs[i], nplanar * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_planar_to_nhwc(dpl, C, B, h, w, dsts[i], Cp, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (flow) {
        CHK(st.in(flow, nfl, "flow planar", &dfl_pl)); CHK(st.out(nfl, "flow", &dfl));
        HIPCHK(launch_planar_to_nhwc(dfl_pl, 2, B, h, w, dfl, 2, c->stream));
    }
    CorrLaunch cl = op_corr_launch(c, 0, B, Cp, h, w);
    cl.ref = dsts[0]; cl.nbr_fut = dsts[1]; cl.nbr_past = dsts[2];
    cl.flow = dfl;
    cl.flow_b = nullptr;
    cl.k = k; cl.out = dcv;
    HIPCHK(launch_warp_costvol(cl, c->stream));
    std::vector<float> rec((size_t)B * hw * kCvRec);
    CHK(st.finish());
    CHK(st.get(rec.data(), dcv, rec.size()));
    // record slots -> the reference's JoinTable order {fwd 81, bwd 81}; the kernel divided by Cp,
    // CostVolMulti.lua:100 divides by N = C
    const float fix = (Cp != C) ? (float)Cp / (float)C : 1.f;
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < 2; ++d)
            for (int ch = 0; ch < 81; ++ch) {
                const int slot = cv_slot(d, ch);
                float *dst = out + ((size_t)b * kND + d * 81 + ch) * hw;
                const float *src = rec.data() + (size_t)b * hw * kCvRec + slot;
                for (size_t i = 0; i < hw; ++i) dst[i] = src[i * kCvRec] * fix;
            }
    return 0;
}
B2F_CATCH("b2f_op_warp_costvol")

int b2f_op_costvol(b2f_ctx *c, const float *ref, const float *frm, int B, int C, int h, int w, int win, int fwd,
                   float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(ref && frm && out));
    if (win < 1 || win % 2 == 0) return fail("b2f_op_costvol: win must be odd");
    const size_t hw = (size_t)h * w;
    if (win == kWin && C % 8 == 0) {
        // the shipped 9x9 window goes through the fused kernel (no warp): one half of its record
        std::vector<float> both((size_t)B * kND * hw);
        CHK(b2f_op_warp_costvol(c, ref, frm, frm, nullptr, 0.f, B, C, h, w, both.data()));
        for (int b = 0; b < B; ++b)
            memcpy(out + (size_t)b * 81 * hw, both.data() + ((size_t)b * kND + (fwd ? 0 : 81)) * hw, 81 * hw * sizeof(float));
        return 0;
    }
    const size_t nin = (size_t)B * C * hw, nout = (size_t)B * win * win * hw;
    float *dpl, *dr, *df, *dcv, *dout;
    CHK(st.in(ref, nin, "planar staging", &dpl)); CHK(st.out(nin, "ref", &dr)); CHK(st.out(nin, "frm", &df));
    CHK(st.out(nout, "cost volume", &dcv)); CHK(st.out(nout, "out", &dout));
    HIPCHK(launch_planar_to_nhwc(dpl, C, B, h, w, dr, C, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the staging buffer is read before frm overwrites it
    HIPCHK(hipMemcpy(dpl, frm, nin * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(launch_planar_to_nhwc(dpl, C, B, h, w, df, C, c->stream));
    HIPCHK(launch_costvol_generic(dr, df, B, C, h, w, win, fwd, dcv, c->stream));
    HIPCHK(launch_nhwc_to_planar(dcv, win * win, win * win, B, h, w, dout, c->stream));
    CHK(st.finish());
    return st.get(out, dout, nout);
}
B2F_CATCH("b2f_op_costvol")

int b2f_op_conv3x3(b2f_ctx *c, const float *x, int B, int Ci, int H, int W, const float *wt, const float *bias,
                   int Co, int stride, int leaky, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && wt && bias && y));
    if (stride != 1 && stride != 2) return fail("b2f_op_conv3x3: stride must be 1 or 2");
    // a one-layer model: packed as pack_all packs a layer, launched as run_conv launches it, on NHWC strides
    PackedConv p;
    p.cout = Co;
    p.chunks[0] = (Ci + kCK - 1) / kCK;
    p.base = base_kernel(Ci, Co, stride == 1, false);
    const int Cp = p.chunks[0] * kCK, Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    // The kernel tests address a layer's kernel at any map size, so the entry leaves the F(4x4) -> F(2x2) fallback of small maps out; with
    // option op_wino_split = 1 (tests) layers of more than 32 outputs take it at every size, one block per 32-output N tile.
    KernelOpts o = *c;
    o.adaptive_kernels = 0;
    o.wino4_min_pixels = o.wino_split_pixels = (c->op_wino_split && Co > 32) ? 0x7fffffff : 0;
    size_t nw = 0;
    place_packings(p, stride == 1, o, &nw);
    std::vector<float> wpk(nw, 0.f);
    fill_packings(p, wt, bias, Ci, nullptr, wpk.data());
    const size_t nx = (size_t)B * Ci * H * W, nxp = (size_t)B * H * W * Cp, ny = (size_t)B * Co * Ho * Wo;
    float *dpl, *dx, *dw, *dy, *dyp;
    CHK(st.in(x, nx, "x planar", &dpl)); CHK(st.out(nxp, "x", &dx)); CHK(st.in(wpk.data(), nw, "weights", &dw));
    CHK(st.out(ny, "y", &dy)); CHK(st.out(ny, "y planar", &dyp));
    HIPCHK(launch_planar_to_nhwc(dpl, Ci, B, H, W, dx, Cp, c->stream));
    ConvLaunch L{};
    L.seg[0] = {dx, (long)((size_t)H * W * Cp), 8, Cp, 0};
    L.out = dy;
    L.out_img_stride = (long)((size_t)Ho * Wo * Co); L.out_chunk_stride = 8; L.out_pix_stride = Co;
    L.H = H; L.W = W; L.stride = stride; L.nimg = B; L.leaky = leaky;
    CHK(launch_layer(c, c->stream, true, p, dw, o, 0, L));   // with option profile: the row names the kernel that ran (tests read the tag)
    HIPCHK(launch_nhwc_to_planar(dy, Co, Co, B, Ho, Wo, dyp, c->stream));
    CHK(st.finish());
    return st.get(y, dyp, ny);
}
B2F_CATCH("b2f_op_conv3x3")

// Conv (kind, level, idx) of the context's own packed table, launched exactly as the forward pass launches it: through run_conv, weights from
// wpk_dev, the kernel by choose_kernel under the context's options with cur_batch = nimg, chunk-planar buffers, profile rows as in a forward.
// x: nimg x Ci x H x W planar in the layer's Torch input order -- for a first decoder layer {cv 162, cs[ref] C_l, flow 2} (pwc.lua:308,334,337) --
// scattered here into the feature segment and the cost-volume record (cv_slot, and the flow at the slots of the decoder's kind, as pack_all maps
// them).  Every packed input channel that the layer's cin_map marks -1 -- the record slots this decoder does not read: the other decoder's
// flow, slots 166 / 167, all six of level 7 -- is filled with the non-zero finite value 1 + op_hole_fill + slot / 256 (option op_hole_fill,
// default 0): the layer's weights there are zero, so the result must not depend on them.  y: nimg x Co x Ho x Wo planar.
// The shipped graph only; feat2.conv1 is launch_conv_first, not run_conv, and is refused.
int b2f_op_layer(b2f_ctx *c, int kind, int level, int idx, int nimg, int H, int W, const float *x, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && y));
    if (!c->g.shipped()) return fail("b2f_op_layer: only the shipped graph (models/pwc.lua with the options of opts.lua) is covered");
    if (nimg < 1 || H < 1 || W < 1) return fail("b2f_op_layer: bad size");
    if (kind == KIND_FEAT && level == 2 && idx == 1) return fail("b2f_op_layer: feat2.conv1 runs in launch_conv_first, not in run_conv");
    const int id = find_conv_id(c, kind, level, idx);
    if (id < 0) return fail("b2f_op_layer: no conv (kind " + std::to_string(kind) + ", level " + std::to_string(level) + ", idx " + std::to_string(idx) + ") in this model");
    if (!c->wpk_dev) return fail("b2f_op_layer: no weights loaded");
    const ConvDesc &d = c->lay[(size_t)id];
    const PackedConv &p = c->packed[(size_t)id];
    PackedConv q;   // the layer's K order, as pack_all derived it: only nseg and chunks are set, cout and base are not
    const std::vector<int> m = layer_cin_map(d, true, q);
    if (q.nseg != p.nseg || q.chunks[0] != p.chunks[0] || (q.nseg == 2 && q.chunks[1] != p.chunks[1])) return fail("b2f_op_layer: the layer's K order is not the packed table's");
    const int stride = (kind == KIND_FEAT && idx == 1) ? 2 : 1, leaky = (kind == KIND_FEAT || idx < 6) ? 1 : 0;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const size_t hw = (size_t)H * W, hwo = (size_t)Ho * Wo;
    // host scatter: segment s is chunk-planar [image][chunk][H][W][8]
    std::vector<float> host;
    ConvSeg segs[2];
    for (int s = 0, k0 = 0; s < p.nseg; k0 += p.chunks[s] * kCK, ++s) {
        const int Cs = p.chunks[s] * kCK;
        host.resize((size_t)nimg * Cs * hw);
        planar_to_cp8(x, (size_t)nimg, d.ci, hw, m.data() + k0, 1.0f + (float)c->op_hole_fill, Cs, host.data());
        // (the arena promises nothing about what lies behind a buffer: here it is the guard's kGuardWord)
        float *dseg;
        CHK(st.in(host.data(), host.size(), s == 0 ? "segment 0" : "segment 1", &dseg));
        segs[s] = cp8_seg(dseg, Cs, hw);
    }
    if (p.nseg == 1) segs[1] = segs[0];
    const size_t ny = (size_t)nimg * ((d.co + 7) / 8 * 8) * hwo;
    float *dy;
    CHK(st.out(ny, "y", &dy));
    HIPCHK(hipDeviceSynchronize());   // the copies ran on the null stream, the layer runs on the context's
    const int batch_before = c->cur_batch;   // run_conv chooses the kernel for a request of cur_batch triplets: nimg for this launch only
    c->cur_batch = nimg;
    const int rc = run_conv_layer(c, c->stream, false, id, segs, nimg, H, W, stride, leaky, dy);
    c->cur_batch = batch_before;
    CHK(rc);
    CHK(st.finish());
    std::vector<float> out(ny);
    CHK(st.get(out.data(), dy, ny));
    cp8_to_planar(out.data(), (size_t)nimg, d.co, hwo, y);
    return 0;
}
B2F_CATCH("b2f_op_layer")

// launch_warp_costvol with the strides of the forward pass: the three maps (B x C x h x w planar here, C a multiple of 8) and the record
// chunk-planar, flow / flow_b (B x 2 x h x w planar here, or NULL) as B x h x w x 2, the context's corr_variant.  rec: the whole record,
// B x 168 x h x w planar in slot order (b2f_internal.h: fwd 0..79 | bwd 0..79 | fwd80 bwd80 u v ub vb 0 0).  The record buffer starts out as NaN
// (kGuardWord, like every buffer of the scope), so a slot the kernel does not write shows.
int b2f_op_cv_record(b2f_ctx *c, const float *ref, const float *nbr_future, const float *nbr_past, const float *flow, const float *flow_b,
                     float k, int B, int C, int h, int w, float *rec) try
{
    OpStage st(c, __func__);
    CHK(st.begin(ref && nbr_future && nbr_past && rec));
    if (B < 1 || C < 8 || C % 8 || h < 1 || w < 1) return fail("b2f_op_cv_record: bad shape (C must be a multiple of 8)");
    const size_t hw = (size_t)h * w, nmap = (size_t)B * C * hw, nrec = (size_t)B * kCvRec * hw, nfl = (size_t)B * 2 * hw;
    float *dmap[3], *dfl[2] = {nullptr, nullptr}, *drec;
    const float *maps[3] = {ref, nbr_future, nbr_past}, *flows[2] = {flow, flow_b};
    std::vector<float> host(std::max(nmap, nrec));
    for (int i = 0; i < 3; ++i) {
        planar_to_cp8(maps[i], (size_t)B, C, hw, nullptr, 0.f, C, host.data());
        CHK(st.in(host.data(), nmap, i == 0 ? "ref" : i == 1 ? "nbr_future" : "nbr_past", &dmap[i]));
    }
    for (int i = 0; i < 2; ++i) {
        if (!flows[i]) continue;
        for (int b = 0; b < B; ++b)
            for (int ch = 0; ch < 2; ++ch)
                for (size_t j = 0; j < hw; ++j) host[((size_t)b * hw + j) * 2 + ch] = flows[i][((size_t)b * 2 + ch) * hw + j];
        CHK(st.in(host.data(), nfl, i == 0 ? "flow" : "flow_b", &dfl[i]));
    }
    CHK(st.out(nrec + 64, "record", &drec));   // the slack the arena gives the record (make_plan); the guard lies behind it, as in the arena
    HIPCHK(hipDeviceSynchronize());
    CorrLaunch cl = op_corr_launch(c, 1, B, C, h, w);
    cl.ref = dmap[0]; cl.nbr_fut = dmap[1]; cl.nbr_past = dmap[2];
    cl.flow = dfl[0]; cl.flow_b = dfl[1];
    cl.k = k; cl.out = drec;
    HIPCHK(launch_warp_costvol(cl, c->stream));
    CHK(st.finish());
    CHK(st.get(host.data(), drec, nrec));
    cp8_to_planar(host.data(), (size_t)B, kCvRec, hw, rec);
    return 0;
}
B2F_CATCH("b2f_op_cv_record")

// The variant launch_warp_costvol would run for a B x C x h x w call under the context's options: choose_corr_variant on the CorrLaunch that
// b2f_op_warp_costvol (layout 0, C padded to a multiple of 8) or b2f_op_cv_record (layout 1) fills through op_corr_launch, no buffers.
int b2f_op_cv_variant(b2f_ctx *c, int B, int C, int h, int w, int layout) try
{
    if (!c) { fail("b2f_op_cv_variant: null argument"); return -1; }
    if (layout != 0 && layout != 1) { fail("b2f_op_cv_variant: layout must be 0 (b2f_op_warp_costvol) or 1 (b2f_op_cv_record)"); return -1; }
    if (B < 1 || C < 1 || h < 1 || w < 1 || (layout == 1 && C % 8)) { fail("b2f_op_cv_variant: bad shape (layout 1: C must be a multiple of 8)"); return -1; }
    if (hipSetDevice(c->device) != hipSuccess) { fail("b2f_op_cv_variant: hipSetDevice failed"); return -1; }
    const CorrLaunch cl = op_corr_launch(c, layout, B, layout == 0 ? (C + 7) / 8 * 8 : C, h, w);
    return choose_corr_variant(cl);
}
catch (const std::exception &e) { fail(std::string("b2f_op_cv_variant: ") + e.what()); return -1; }
catch (...) { fail("b2f_op_cv_variant: unknown exception"); return -1; }

int b2f_op_conv_head16(b2f_ctx *c, const float *x, int B, int H, int W, const float *w1, const float *b1, const float *w2,
                       const float *b2, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && w1 && b1 && w2 && b2 && y));
    if (B < 1 || H < 1 || W < 1) return fail("b2f_op_conv_head16: bad size");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    std::vector<float> p1(c16_wpk_floats()), pb1(32), p2(c16s2_wpk_floats()), pb2(32);
    c16_pack_weights(w1, b1, 16, nullptr, p1.data(), pb1.data());
    c16s2_pack_weights(w2, b2, 16, nullptr, p2.data(), pb2.data());
    const size_t nx = (size_t)B * 16 * H * W, ny = (size_t)B * 32 * Ho * Wo;
    float *dpl, *dx, *dw1, *db1, *dw2, *db2, *dy, *dyp;
    CHK(st.in(x, nx, "x planar", &dpl)); CHK(st.out(nx, "x", &dx));
    CHK(st.in(p1.data(), p1.size(), "w1", &dw1)); CHK(st.in(pb1.data(), 32, "b1", &db1));
    CHK(st.in(p2.data(), p2.size(), "w2", &dw2)); CHK(st.in(pb2.data(), 32, "b2", &db2));
    CHK(st.out(ny, "y", &dy)); CHK(st.out(ny, "y planar", &dyp));
    HIPCHK(launch_planar_to_nhwc(dpl, 16, B, H, W, dx, 16, c->stream));
    HeadLaunch hl;
    hl.in = dx; hl.in_img_stride = (long)((size_t)H * W * 16); hl.in_chunk_stride = 8; hl.in_pix_stride = 16;
    hl.H1 = H; hl.W1 = W;
    hl.w1 = dw1; hl.b1 = db1; hl.w2 = dw2; hl.b2 = db2;
    hl.out = dy; hl.out_img_stride = (long)((size_t)Ho * Wo * 32); hl.out_chunk_stride = 8; hl.out_pix_stride = 32;
    hl.Ho = Ho; hl.Wo = Wo; hl.nimg = B;
    if (!head16_supported(hl)) return fail("b2f_op_conv_head16: unsupported shape");
    HIPCHK(launch_conv_head16(hl, c->stream));
    HIPCHK(launch_nhwc_to_planar(dy, 32, 32, B, Ho, Wo, dyp, c->stream));
    CHK(st.finish());
    return st.get(y, dyp, ny);
}
B2F_CATCH("b2f_op_conv_head16")

// The first pyramid conv as the forward launches it (launch_conv_first, pwc.lua:59: conv(3, 16, s2) + LeakyReLU on each of the three
// frames, after ColorNormalize when normalize != 0).  x: B x 9 x H x W planar, frame f in channels 3 f .. 3 f + 2, H and W even (the
// kernel computes H / 2 x W / 2 outputs); wt: 16 x 3 x 3 x 3, bias: 16; y: 3 B x 16 x H/2 x W/2 planar, image f * B + b.
int b2f_op_conv_first(b2f_ctx *c, const float *x, int B, int H, int W, int normalize, const float *wt, const float *bias, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && wt && bias && y));
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail("b2f_op_conv_first: H and W must be even and at least 2");
    const size_t hwo = (size_t)(H / 2) * (W / 2), nx = (size_t)B * 9 * H * W, ny = (size_t)3 * B * 16 * hwo;
    std::vector<float> wp(27 * 16), out(ny);
    pack_first_conv(wt, wp.data());
    float *dx, *dw, *db, *dy;
    CHK(st.in(x, nx, "x", &dx)); CHK(st.in(wp.data(), wp.size(), "weights", &dw)); CHK(st.in(bias, 16, "bias", &db)); CHK(st.out(ny, "y", &dy));
    HIPCHK(launch_conv_first(dx, normalize ? 1 : 0, B, H, W, dw, db, dy, c->stream));
    CHK(st.finish());
    CHK(st.get(out.data(), dy, ny));
    cp8_to_planar(out.data(), (size_t)3 * B, 16, hwo, y);
    return 0;
}
B2F_CATCH("b2f_op_conv_first")

// ---- the forward's small kernels (b2f_glue.hip, b2f_seq.hip), one entry per launcher on the caller's own strides: the host hands over the
// records as the forward lays them out (e.g. 8-float flow records whose slots 2..7 hold NaN), nothing is repacked on the way in.
// tests/test_gpu_glue_float64.py

int b2f_op_upsample_flow2x_ex(b2f_ctx *c, const float *x, int ps, int B, int h, int w, int planar, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && y));
    if (!small_dims(B, h, w) || ps < 2 || (ps & 1) || ps > 64) return fail("b2f_op_upsample_flow2x_ex: bad shape (B, h, w >= 1, ps even in 2..64)");
    const size_t nx = (size_t)B * h * w * ps, ny = (size_t)B * 8 * h * w;
    float *dx, *dy;
    CHK(st.in(x, nx, "x", &dx)); CHK(st.out(ny, "y", &dy));
    if (planar) HIPCHK(launch_upsample_flow2x_planar(dx, ps, B, h, w, dy, c->stream));
    else HIPCHK(launch_upsample_flow2x(dx, ps, B, h, w, dy, c->stream));
    CHK(st.finish());
    return st.get(y, dy, ny);
}
B2F_CATCH("b2f_op_upsample_flow2x_ex")

int b2f_op_softmax_nearest4(b2f_ctx *c, const float *logits, int ps, int B, int h, int w, float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(logits && out));
    if (!small_dims(B, h, w) || ps < 2 || (ps & 1) || ps > 64) return fail("b2f_op_softmax_nearest4: bad shape (B, h, w >= 1, ps even in 2..64)");
    const size_t nx = (size_t)B * h * w * ps, ny = (size_t)B * 32 * h * w;
    float *dx, *dy;
    CHK(st.in(logits, nx, "logits", &dx)); CHK(st.out(ny, "out", &dy));
    HIPCHK(launch_softmax_nearest4_planar(dx, ps, B, h, w, dy, c->stream));
    CHK(st.finish());
    return st.get(out, dy, ny);
}
B2F_CATCH("b2f_op_softmax_nearest4")

int b2f_op_avgpool2(b2f_ctx *c, const float *x, int nimg, int H, int W, int C, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && y));
    if (!small_dims(nimg, H, W) || H < 2 || W < 2 || C < 4 || (C & 3) || C > 1024) return fail("b2f_op_avgpool2: bad shape (H, W >= 2, C a multiple of 4)");
    const size_t nx = (size_t)nimg * H * W * C, ny = (size_t)nimg * (H / 2) * (W / 2) * C;
    float *dx, *dy;
    CHK(st.in(x, nx, "x", &dx)); CHK(st.out(ny, "y", &dy));
    HIPCHK(launch_avgpool2_nhwc(dx, nimg, H, W, C, dy, c->stream));
    CHK(st.finish());
    return st.get(y, dy, ny);
}
B2F_CATCH("b2f_op_avgpool2")

int b2f_op_pack_input(b2f_ctx *c, const float *x, int normalize, int B, int H, int W, float *img) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && img));
    if (!small_dims(B, H, W)) return fail("b2f_op_pack_input: bad shape");
    const size_t nx = (size_t)B * 9 * H * W, ny = (size_t)3 * B * H * W * kImgC;
    float *dx, *dy;
    CHK(st.in(x, nx, "x", &dx)); CHK(st.out(ny, "img", &dy));
    HIPCHK(launch_pack_input(dx, normalize ? 1 : 0, B, H, W, dy, c->stream));
    CHK(st.finish());
    return st.get(img, dy, ny);
}
B2F_CATCH("b2f_op_pack_input")

int b2f_op_warp_image(b2f_ctx *c, int which, const void *in, int in_kind, int frame, const float *flow, float k, int B, int H, int W,
                      float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(in && flow && out));
    if (!small_dims(B, H, W)) return fail("b2f_op_warp_image: bad shape");
    if (which < 0 || which > 2) return fail("b2f_op_warp_image: which must be 0 (warp_image_planar), 1 (warp_input_planar) or 2 (warp_input_seq)");
    if (which == 1 && (frame < 0 || frame > 2 || (in_kind != B2F_IN_NORMALIZED && in_kind != B2F_IN_UNIT)))
        return fail("b2f_op_warp_image: warp_input_planar takes frame 0..2 and float samples");
    if (which == 2 && in_kind != B2F_IN_NORMALIZED && in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8) return fail("b2f_op_warp_image: bad in_kind");
    const size_t hw = (size_t)H * W, samples = which == 0 ? (size_t)B * hw * kImgC : (which == 1 ? (size_t)B * 9 * hw : (size_t)B * 3 * hw);
    const size_t bytes = samples * ((which == 2 && in_kind == B2F_IN_U8) ? 1 : sizeof(float)), no = (size_t)B * 3 * hw;
    unsigned char *di;
    float *df, *dout;
    CHK(st.in((const unsigned char *)in, bytes, "in", &di)); CHK(st.in(flow, (size_t)B * 2 * hw, "flow", &df)); CHK(st.out(no, "out", &dout));
    if (which == 0) HIPCHK(launch_warp_image_planar((const float *)di, df, k, B, H, W, dout, c->stream));
    else if (which == 1) HIPCHK(launch_warp_input_planar((const float *)di, in_kind == B2F_IN_UNIT ? 1 : 0, frame, df, k, B, H, W, dout, c->stream));
    else HIPCHK(launch_warp_input_seq(di, in_kind, df, k, B, H, W, dout, c->stream));
    CHK(st.finish());
    return st.get(out, dout, no);
}
B2F_CATCH("b2f_op_warp_image")

int b2f_op_conv_first_seq(b2f_ctx *c, const void *x, int in_kind, int T, int H, int W, const float *wt, const float *bias, float *y) try
{
    OpStage st(c, __func__);
    CHK(st.begin(x && wt && bias && y));
    if (!small_dims(T, H, W) || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail("b2f_op_conv_first_seq: H and W must be even and at least 2");
    if (in_kind != B2F_IN_NORMALIZED && in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8) return fail("b2f_op_conv_first_seq: bad in_kind");
    const size_t hwo = (size_t)(H / 2) * (W / 2), nx = (size_t)T * 3 * H * W, ny = (size_t)T * 16 * hwo;
    std::vector<float> wp(27 * 16), out(ny);
    pack_first_conv(wt, wp.data());
    unsigned char *dx;
    float *dw, *db, *dy;
    CHK(st.in((const unsigned char *)x, nx * (in_kind == B2F_IN_U8 ? 1 : sizeof(float)), "x", &dx));
    CHK(st.in(wp.data(), wp.size(), "weights", &dw)); CHK(st.in(bias, 16, "bias", &db)); CHK(st.out(ny, "y", &dy));
    HIPCHK(launch_conv_first_seq(dx, in_kind, T, H, W, dw, db, dy, c->stream));
    CHK(st.finish());
    CHK(st.get(out.data(), dy, ny));
    cp8_to_planar(out.data(), (size_t)T, 16, hwo, y);
    return 0;
}
B2F_CATCH("b2f_op_conv_first_seq")

int b2f_op_layout(b2f_ctx *c, int which, const float *in, int C, int pix_stride, int B, int h, int w, float *out) try
{
    OpStage st(c, __func__);
    CHK(st.begin(in && out));
    if (!small_dims(B, h, w) || C < 1 || C > 4096) return fail("b2f_op_layout: bad shape");
    if (which < 0 || which > 2) return fail("b2f_op_layout: which must be 0 (nhwc_to_planar), 1 (cp8_to_planar) or 2 (planar_to_nhwc)");
    if (which != 1 && (pix_stride < C || pix_stride > 8192)) return fail("b2f_op_layout: pix_stride must be at least C");
    const size_t hw = (size_t)h * w, planar = (size_t)B * C * hw, nhwc = (size_t)B * hw * pix_stride, cp8 = (size_t)B * ((C + 7) / 8) * hw * 8;
    const size_t ni = which == 0 ? nhwc : (which == 1 ? cp8 : planar), no = which == 2 ? nhwc : planar;
    float *di, *dout;
    CHK(st.in(in, ni, "in", &di)); CHK(st.out(no, "out", &dout));
    if (which == 0) HIPCHK(launch_nhwc_to_planar(di, pix_stride, C, B, h, w, dout, c->stream));
    else if (which == 1) HIPCHK(launch_cp8_to_planar(di, C, B, h, w, dout, c->stream));
    else HIPCHK(launch_planar_to_nhwc(di, C, B, h, w, dout, pix_stride, c->stream));
    CHK(st.finish());
    return st.get(out, dout, no);
}
B2F_CATCH("b2f_op_layout")

}  // extern "C"
