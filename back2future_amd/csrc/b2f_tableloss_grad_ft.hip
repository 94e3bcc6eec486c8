// The gradient of the Soft models' fine-tuning objective (README.md:89-102) with respect to the output table on the device:
// table_loss_grad_kernel (b2f_tableloss_grad.hip) with SecondOrderSmoothnessCriterion for the flows and / or OBGCCriterion for the
// photometric term where the options ask for them.  Same shape: one launch per level over the same capped (blocks, n) grid, a thread
// covers four consecutive pixels of a row through load_px / store_px, no LDS, no atomics, the halo rows through the cache.  The
// stencil is wider: S2 of a pixel takes q of its four neighbours, so the flows and the reference are read on the radius-2 cross
// (eight columns of the row, the two rows above and the two below); OBGCC takes the warped planes and the reference on the
// five-point cross.  To hold the registers down the planes go one after another:
//   1. the reference, channel by channel, into the 23 sums of |R(a) - R(b)| over the pairs of the cross (7 along the row, 4 x 4 over
//      the rows).  Both kinds of contrast weight are functions of those sums: 13 first-order weights (for the occlusions, and for
//      the flows without -smooth_second_order) and 18 second-order ones (6 columns, 3 rows x 4), each exponential computed once and
//      shared by every addend and plane that uses it;
//   2. the flows, plane by plane; 3. the occlusions' first-order smoothness; 4. the photometric term, direction by direction and
//      channel by channel, with the five P1 sums of a pixel carried over the channels; 5. the occlusions' elements.
// The per-element functions are those of b2f_tableloss_grad.h and b2f_tableloss_grad_ft.h, which the host entry
// (b2f_table_loss_grad_ft_host) shares, so both give the same bits.
#include "b2f_ctx.h"
#include "b2f_tableloss_grad_ft.h"
#include "b2f_tableloss_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px, store_px)
constexpr int kThreads = kLossThreads;

// the radius-2 cross of a group in one plane: cur[2..5] the group, cur[0..1] / cur[6..7] the two pixels left / right of it, up2, up1,
// low1, low2 the rows y - 2 .. y + 2 over the group's columns; what does not exist is 0 and is not read
__device__ __forceinline__ void load_cross2(const float *pl, const Group &g, float *cur, float *up2, float *up1, float *low1, float *low2)
{
#pragma unroll
    for (int k = 0; k < kPx; ++k) up2[k] = up1[k] = low1[k] = low2[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < kPx + 4; ++k) cur[k] = 0.0f;
    load_px(pl + g.i0, g.n, cur + 2);
    if (g.x0 > 0) {   // x0 is a multiple of kPx: both exist
        cur[0] = pl[g.i0 - 2];
        cur[1] = pl[g.i0 - 1];
    }
    if (g.x0 + kPx < g.w) cur[kPx + 2] = pl[g.i0 + kPx];
    if (g.x0 + kPx + 1 < g.w) cur[kPx + 3] = pl[g.i0 + kPx + 1];
    if (g.u2) load_px(pl + g.i0 - 2 * (size_t)g.w, g.n, up2);
    if (g.u1) load_px(pl + g.i0 - g.w, g.n, up1);
    if (g.d1) load_px(pl + g.i0 + g.w, g.n, low1);
    if (g.d2) load_px(pl + g.i0 + 2 * (size_t)g.w, g.n, low2);
}

// the contrast weights of a group: first-order wx[i] of the pair of columns x0 - 1 + i and x0 + i, wyc / wyu of the pairs with the row
// below / above; second-order w2x[i] of column x0 - 1 + i, w2y[r] of row y - 1 + r.  A weight whose pixels do not all exist is not used.
struct Weights {
    double wx[kPx + 1], wyc[kPx], wyu[kPx];
    double w2x[kPx + 2], w2y[3][kPx];
};

// S or S2 of the group's four pixels in one plane of a flow
template <bool Second>
__device__ __forceinline__ void smooth_flow4(const float *pl, const Group &g, const Weights &wt, double *S)
{
    float cur[kPx + 4], up2[kPx], up1[kPx], low1[kPx], low2[kPx];
    if (Second) {
        load_cross2(pl, g, cur, up2, up1, low1, low2);
        double qx[kPx + 2];   // of column x0 - 1 + i
#pragma unroll
        for (int i = 0; i < kPx + 2; ++i) qx[i] = grad2_q(g.x0 - 1 + i >= 1 && g.x0 + i < g.w, cur[i], cur[i + 1], cur[i + 2], wt.w2x[i]);
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const double qu = grad2_q(g.u2 && g.u1, up2[k], up1[k], cur[k + 2], wt.w2y[0][k]);     // row y - 1 is interior: y - 2 >= 0 (y < h)
            const double qc = grad2_q(g.u1 && g.d1, up1[k], cur[k + 2], low1[k], wt.w2y[1][k]);
            const double qd = grad2_q(g.d2, cur[k + 2], low1[k], low2[k], wt.w2y[2][k]);           // row y + 1 is interior: y + 2 < h (y >= 0)
            S[k] = grad2_s(qc, qx[k + 1], qd, qx[k + 2], qu, qx[k]);
        }
    } else {
        load_cross<true>(pl, g, cur, up1, low1);
        smooth4<false>(cur, up1, low1, g, wt.wx, wt.wyc, wt.wyu, S);
    }
}

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  FlowOnly: phases 1 and 2 alone -- the
// flow planes of a table whose occlusion and image planes table_loss_grad_ssim_kernel writes (b2f_tableloss_grad_ssim.hip); gp.o,
// gp.iw1 and gp.iw3 are not touched.
template <bool Past, bool Second, bool FlowOnly>
__global__ void __launch_bounds__(kThreads) table_loss_grad_ft_kernel(LevelPtrs lp, GradPtrs gp, int h, int w, float kd, GradFtCoef kf)
{
    const GradCoef &k = kf.k;
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const float *R = lp.ref + b * lp.ref_stride;
    const float *f = lp.f + b * 2 * hw, *p = Past ? lp.p + b * 2 * hw : nullptr, *o = lp.o + b * 2 * hw;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    float *gf = gp.f + b * 2 * hw, *gpp = Past ? gp.p + b * 2 * hw : nullptr, *go = gp.o + b * 2 * hw;
    float *giw[2] = {gp.iw1 + b * 3 * hw, gp.iw3 + b * 3 * hw};
    const bool on_s = (k.on & kGradSmooth) != 0, on_cv = Past && (k.on & kGradConstVel) != 0, on_p = !FlowOnly && (k.on & kGradPhoto) != 0,
               on_so = !FlowOnly && (k.on & kGradSmoothOcc) != 0, obgcc = (kf.ft & kGradFtObgcc) != 0;
    const bool want_w1 = on_so || (!Second && on_s), want_w2 = Second && on_s;
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const Group g = group_at(y, x0, h, w);
        // 1. the reference: the sums of the pairs, then the weights
        Weights wt;
        if (want_w1 || want_w2) {
            double ax[kPx + 3] = {};    // the pair of columns x0 - 2 + i and x0 - 1 + i
            double ay[4][kPx] = {};     // the pair of rows y - 2 + r and y - 1 + r
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float cur[kPx + 4], up2[kPx], up1[kPx], low1[kPx], low2[kPx];
                if (want_w2) {
                    load_cross2(R + (size_t)c * hw, g, cur, up2, up1, low1, low2);
                } else {
                    load_cross<true>(R + (size_t)c * hw, g, cur + 1, up1, low1);
                    cur[0] = cur[kPx + 3] = 0.0f;
#pragma unroll
                    for (int q = 0; q < kPx; ++q) up2[q] = low2[q] = 0.0f;
                }
#pragma unroll
                for (int i = 0; i < kPx + 3; ++i) ax[i] = grad_abs3_add(ax[i], c == 0, cur[i], cur[i + 1]);
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    ay[0][q] = grad_abs3_add(ay[0][q], c == 0, up2[q], up1[q]);
                    ay[1][q] = grad_abs3_add(ay[1][q], c == 0, up1[q], cur[q + 2]);
                    ay[2][q] = grad_abs3_add(ay[2][q], c == 0, cur[q + 2], low1[q]);
                    ay[3][q] = grad_abs3_add(ay[3][q], c == 0, low1[q], low2[q]);
                }
            }
            if (want_w1) {
#pragma unroll
                for (int i = 0; i <= kPx; ++i) wt.wx[i] = grad_weight_sum(ax[i + 1]);
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    wt.wyc[q] = grad_weight_sum(ay[2][q]);
                    wt.wyu[q] = grad_weight_sum(ay[1][q]);
                }
            }
            if (want_w2) {
#pragma unroll
                for (int i = 0; i < kPx + 2; ++i) wt.w2x[i] = grad2_weight_sums(ax[i], ax[i + 1]);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < kPx; ++q) wt.w2y[r][q] = grad2_weight_sums(ay[r][q], ay[r + 1][q]);
            }
        }
        // the centres of the flows: the two targets' `inside` (bit q of ins[d]) and the constant-velocity term
        unsigned ins[2] = {0u, 0u};
        double cv[kPx][2];
        {
            float fc[2][kPx], pc[2][kPx];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int q = 0; q < kPx; ++q) fc[c][q] = pc[c][q] = 0.0f;
                load_px(f + (size_t)c * hw + g.i0, g.n, fc[c]);
                if (Past) load_px(p + (size_t)c * hw + g.i0, g.n, pc[c]);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                cv[q][0] = cv[q][1] = 0.0;
                if (on_cv) grad_const_vel(fc[0][q], fc[1][q], pc[0][q], pc[1][q], cv[q]);
                if (on_p) {
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        const bool pf = d == 0 && Past;   // OBGCCriterion.lua:226-230, OBCCriterion.lua:166-170
                        // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not stored
                        const WarpTaps tp = warp_taps(pf ? pc[0][q] : fc[0][q], pf ? pc[1][q] : fc[1][q], d == 0 ? -kd : kd, q < g.n ? x0 + q : x0, y, w, h);
                        if (tp.inside) ins[d] |= 1u << q;
                    }
                }
            }
        }
        // 2. the flows
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float out[kPx];
            double S[kPx] = {0.0, 0.0, 0.0, 0.0};
            if (on_s) smooth_flow4<Second>(f + (size_t)c * hw, g, wt, S);
#pragma unroll
            for (int q = 0; q < kPx; ++q) out[q] = grad_flow(k, S[q], cv[q][c], Past, false);
            store_px(gf + (size_t)c * hw + g.i0, g.n, out);
            if (Past) {
                if (on_s) smooth_flow4<Second>(p + (size_t)c * hw, g, wt, S);
#pragma unroll
                for (int q = 0; q < kPx; ++q) out[q] = grad_flow(k, S[q], cv[q][c], true, true);
                store_px(gpp + (size_t)c * hw + g.i0, g.n, out);
            }
        }
        if (FlowOnly) continue;
        // 3. the occlusions: their centres and S with the quadratic penalty
        float oc[2][kPx];
        double So[2][kPx];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float cur[kPx + 2], up[kPx], low[kPx];
#pragma unroll
            for (int q = 0; q < kPx; ++q) So[c][q] = 0.0;
            if (on_so) {
                load_cross<true>(o + (size_t)c * hw, g, cur, up, low);
                smooth4<true>(cur, up, low, g, wt.wx, wt.wyc, wt.wyu, So[c]);
            } else {
#pragma unroll
                for (int q = 0; q < kPx; ++q) cur[q + 1] = 0.0f;
                load_px(o + (size_t)c * hw + g.i0, g.n, cur + 1);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) oc[c][q] = cur[q + 1];
        }
        // 4. the photometric term: G_iw_d, and PO for the occlusions (po[c][q] = PO_c: direction d fills channel 1 - d)
        double po[2][kPx];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            double sums[kPx][5];
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                po[1 - d][q] = 0.0;
#pragma unroll
                for (int t = 0; t < 5; ++t) sums[q][t] = 0.0;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float out[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (on_p && obgcc) {
                    float ic[kPx + 2], iu[kPx], il[kPx], rc[kPx + 2], ru[kPx], rl[kPx];
                    load_cross<true>(iw[d] + (size_t)c * hw, g, ic, iu, il);
                    load_cross<true>(R + (size_t)c * hw, g, rc, ru, rl);
#pragma unroll
                    for (int q = 0; q < kPx; ++q) {
                        const bool has_l = x0 + q > 0, has_r = x0 + q + 1 < w;
                        if (ins[d] >> q & 1u) {
                            ObgccErr e;
                            e.d = (double)ic[q + 1] - (double)rc[q + 1];
                            e.ey = obgcc_e(g.d1, ic[q + 1], il[q], rc[q + 1], rl[q]);
                            e.eyu = g.u1 ? obgcc_e(true, iu[q], ic[q + 1], ru[q], rc[q + 1]) : 0.0;
                            e.ex = obgcc_e(has_r, ic[q + 1], ic[q + 2], rc[q + 1], rc[q + 2]);
                            e.exl = has_l ? obgcc_e(true, ic[q], ic[q + 1], rc[q], rc[q + 1]) : 0.0;
                            out[q] = obgcc_image(kf, g.u1, has_l, e, oc[1 - d][q]);
                            obgcc_p1_add(kf, g.u1, has_l, e, c == 0, sums[q]);
                        }
                    }
                } else if (on_p) {   // OBCC, channel by channel: grad_photo of b2f_tableloss_grad.h
                    float wv[kPx] = {0.0f, 0.0f, 0.0f, 0.0f}, rv[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
                    load_px(iw[d] + (size_t)c * hw + g.i0, g.n, wv);
                    load_px(R + (size_t)c * hw + g.i0, g.n, rv);
#pragma unroll
                    for (int q = 0; q < kPx; ++q)
                        if (ins[d] >> q & 1u) out[q] = obcc_image(k, wv[q], rv[q], oc[1 - d][q], c == 0, &sums[q][0]);
                }
                store_px(giw[d] + (size_t)c * hw + g.i0, g.n, out);
            }
            if (on_p) {
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    const bool has_l = x0 + q > 0;
                    po[1 - d][q] = !(ins[d] >> q & 1u) ? 1.0 : obgcc ? obgcc_po(kf, g.u1, has_l, sums[q]) : sums[q][0];
                }
            }
        }
        // 5. the occlusions
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float out[kPx];
#pragma unroll
            for (int q = 0; q < kPx; ++q) out[q] = grad_occ(k, po[c][q], So[c][q], oc[1 - c][q]);
            store_px(go + (size_t)c * hw + g.i0, g.n, out);
        }
    }
}

}  // namespace

// one level's launch of an instantiation
template <bool Past, bool Second, bool FlowOnly>
static void launch_level(const LossLevel &v, const GradFtCoef &kf, hipStream_t s)
{
    hipLaunchKernelGGL((table_loss_grad_ft_kernel<Past, Second, FlowOnly>), v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, kf);
}

hipError_t launch_table_loss_grad_ft(const float *const *table, float *const *grad, int L, bool past, int n, int H, int W, const float *ref,
                                     size_t ref_stride, const float *pyr, double flow_scale, const GradFtCoef *coef, hipStream_t s, bool flow_only)
{
    LossLevel lv[kLossMaxLevels];
    if (!grad || !coef || !loss_levels(table, grad, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, lv)) return hipErrorInvalidValue;
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        const bool second = (coef[j].ft & kGradFtSecond) != 0;
        if (flow_only) {
            if (past && second) launch_level<true, true, true>(v, coef[j], s);
            else if (past) launch_level<true, false, true>(v, coef[j], s);
            else if (second) launch_level<false, true, true>(v, coef[j], s);
            else launch_level<false, false, true>(v, coef[j], s);
        } else if (past && second) launch_level<true, true, false>(v, coef[j], s);
        else if (past) launch_level<true, false, false>(v, coef[j], s);
        else if (second) launch_level<false, true, false>(v, coef[j], s);
        else launch_level<false, false, false>(v, coef[j], s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f
