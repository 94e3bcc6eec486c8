// The gradient table with the photometric terms that do not mask occlusions (criterions/MBCCriterion.lua:104-186,
// criterions/MSSIML1Criterion.lua:155-261) on the device: the image planes of a level, and its occlusion planes where the occlusions'
// smoothness or prior has a weight (the photometric criterion gives them exactly zero: gradInput[1]:fill(0); without a term the launcher
// sets them to zero with a memset).  The flow planes do not depend on the photometric criterion; table_loss_grad_ft_kernel's FlowOnly
// instantiations write them (b2f_tableloss_grad_ft.hip), so every element of the table is written exactly once, from fp64.  Same shape as
// the family: one launch per level over the capped (blocks, n) grid, a thread covers four consecutive pixels of a row through load_px /
// store_px (16-byte accesses where the address allows, scalar tails), no LDS, no atomics, no read-modify-write, the halo rows through the
// cache.  Per group:
//   1. where the occlusions have a term: the reference's first-order contrast weights, the occlusions' S with the quadratic penalty and
//      their elements, as table_loss_grad_ssim_kernel forms them;
//   2. the two targets' `inside`;
//   3. BCC: the raw difference of every channel through the penalty's derivative; SSIM: T_c on table_loss_ssim_kernel's window
//      machinery (b2f_tableloss_ssim_dev.h), one channel at a time, the loop rolled, the reference's window sums once
//      for both directions.
// The per-element functions are those of b2f_tableloss_plain.h, which the host entry (b2f_table_loss_grad_plain_host) shares, so both
// give the same bits.
#include "b2f_ctx.h"
#include "b2f_tableloss_grad_ft.h"
#include "b2f_tableloss_plain.h"
#include "b2f_tableloss_ssim_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px, store_px)
constexpr int kThreads = kLossThreads;
constexpr int kCols = kSsimCols;
constexpr int kRec = B2F_LOSS_PLAIN_WORDS;

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  Ssim: the criterion is SSIM / SSIML1 and
// rec is the record of image 0 at this level, image b `rec_stride` words further, words RANGE_USED holding the range; else BCC, and rec
// is not read.
template <bool Past, bool Ssim>
__global__ void __launch_bounds__(kThreads) table_loss_grad_plain_kernel(LevelPtrs lp, GradPtrs gp, int h, int w, float kd, GradPlainCoef kp,
                                                                         const unsigned long long *rec, size_t rec_stride)
{
#pragma clang fp contract(off)
    const GradCoef &k = kp.s.k;
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const float *R = lp.ref + b * lp.ref_stride;
    const float *fl[2] = {(Past ? lp.p : lp.f) + b * 2 * hw, lp.f + b * 2 * hw};   // the flow of the direction (MBCCriterion.lua:156-164)
    const float *o = lp.o + b * 2 * hw;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    float *go = gp.o + b * 2 * hw;
    float *giw[2] = {gp.iw1 + b * 3 * hw, gp.iw3 + b * 3 * hw};
    const bool on_p = (k.on & kGradPhoto) != 0, on_so = (k.on & kGradSmoothOcc) != 0, on_o = grad_plain_occ_on(k);
    SsimRange rg = {0.0, 0.0, false};
    if (Ssim && on_p) {
        const unsigned long long *own = rec + b * rec_stride;
        rg = ssim_range(__uint_as_float((unsigned)own[B2F_LOSS_PLAIN_RANGE_USED]), __uint_as_float((unsigned)own[B2F_LOSS_PLAIN_RANGE_USED + 1]));
    }
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const Group g = group_at(y, x0, h, w);
        // 1. the occlusions, where they have a term
        if (on_o) {
            float oc[2][kPx];
            double So[2][kPx];
            if (on_so) {
                double ax[kPx + 1] = {}, ayc[kPx] = {}, ayu[kPx] = {};   // the pairs of columns x0 - 1 + i and x0 + i, of the rows y / y + 1 and y - 1 / y
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float cur[kPx + 2], up[kPx], low[kPx];
                    load_cross<true>(R + (size_t)c * hw, g, cur, up, low);
#pragma unroll
                    for (int i = 0; i <= kPx; ++i) ax[i] = grad_abs3_add(ax[i], c == 0, cur[i], cur[i + 1]);
#pragma unroll
                    for (int q = 0; q < kPx; ++q) {
                        ayc[q] = grad_abs3_add(ayc[q], c == 0, cur[q + 1], low[q]);
                        ayu[q] = grad_abs3_add(ayu[q], c == 0, up[q], cur[q + 1]);
                    }
                }
                double wx[kPx + 1], wyc[kPx], wyu[kPx];
#pragma unroll
                for (int i = 0; i <= kPx; ++i) wx[i] = grad_weight_sum(ax[i]);
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    wyc[q] = grad_weight_sum(ayc[q]);
                    wyu[q] = grad_weight_sum(ayu[q]);
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    float cur[kPx + 2], up[kPx], low[kPx];
                    load_cross<true>(o + (size_t)c * hw, g, cur, up, low);
                    smooth4<true>(cur, up, low, g, wx, wyc, wyu, So[c]);
#pragma unroll
                    for (int q = 0; q < kPx; ++q) oc[c][q] = cur[q + 1];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int q = 0; q < kPx; ++q) {
                        oc[c][q] = 0.0f;
                        So[c][q] = 0.0;
                    }
                    load_px(o + (size_t)c * hw + g.i0, g.n, oc[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float out[kPx];
#pragma unroll
                for (int q = 0; q < kPx; ++q) out[q] = grad_plain_occ(k, So[c][q], oc[1 - c][q]);
                store_px(go + (size_t)c * hw + g.i0, g.n, out);
            }
        }
        // 2. + 3. the photometric term: G_iw_d
        if (on_p) {
            unsigned ins[2] = {0u, 0u};   // bit q of ins[d]: the target of pixel q in direction d is inside
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                float fv[2][kPx];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int q = 0; q < kPx; ++q) fv[c][q] = 0.0f;
                    load_px(fl[d] + (size_t)c * hw + g.i0, g.n, fv[c]);
                }
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not stored
                    const WarpTaps tp = warp_taps(fv[0][q], fv[1][q], d == 0 ? -kd : kd, q < g.n ? x0 + q : x0, y, w, h);
                    if (tp.inside) ins[d] |= 1u << q;
                }
            }
            if (Ssim) {
                const size_t up = g.u1 ? (size_t)w : 0, down = g.d1 ? (size_t)w : 0;   // the clamped rows above and below
                const bool before = x0 > 0, more = x0 + kPx < w;
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    double ty[3][kCols], mu_y[kPx], gyy[kPx];
                    load_rows(R + (size_t)c * hw, g.i0, up, down, g.n, before, more, rg, ty);
                    window4(ty, nullptr, mu_y);
                    window4(ty, ty, gyy);
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        double tx[3][kCols], mu_x[kPx], gxx[kPx], gxy[kPx];
                        load_rows(iw[d] + (size_t)c * hw, g.i0, up, down, g.n, before, more, rg, tx);
                        window4(tx, nullptr, mu_x);
                        window4(tx, tx, gxx);
                        window4(tx, ty, gxy);
                        float out[kPx];
#pragma unroll
                        for (int q = 0; q < kPx; ++q) {
                            const GradSsimChannel ch = grad_ssim_channel(kp.s, tx[1][q + 1], ty[1][q + 1], mu_x[q], mu_y[q], gxx[q], gyy[q], gxy[q]);
                            out[q] = grad_plain_ssim(kp, (ins[d] >> q & 1u) != 0u, ch.t);
                        }
                        store_px(giw[d] + (size_t)c * hw + g.i0, g.n, out);
                    }
                }
            } else {
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    float rv[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
                    load_px(R + (size_t)c * hw + g.i0, g.n, rv);
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        float wv[kPx] = {0.0f, 0.0f, 0.0f, 0.0f}, out[kPx];
                        load_px(iw[d] + (size_t)c * hw + g.i0, g.n, wv);
#pragma unroll
                        for (int q = 0; q < kPx; ++q) out[q] = grad_plain_bcc(kp, (ins[d] >> q & 1u) != 0u, wv[q], rv[q]);
                        store_px(giw[d] + (size_t)c * hw + g.i0, g.n, out);
                    }
                }
            }
        } else {
            const float zero[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int c = 0; c < 3; ++c) store_px(giw[d] + (size_t)c * hw + g.i0, g.n, zero);
        }
    }
}

}  // namespace

hipError_t launch_table_loss_grad_plain(const float *const *table, float *const *grad, int L, bool past, int n, int H, int W, const float *ref,
                                        size_t ref_stride, const float *pyr, double flow_scale, const GradPlainCoef *coef, const unsigned long long *rec,
                                        hipStream_t s)
{
    LossLevel lv[kLossMaxLevels];
    if (!grad || !coef || !loss_levels(table, grad, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, lv)) return hipErrorInvalidValue;
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        const bool ssim = (coef[j].pl & kGradPlainSsim) != 0;
        if (ssim && (coef[j].s.k.on & kGradPhoto) && !rec) return hipErrorInvalidValue;
        const unsigned long long *r = rec ? rec + (size_t)j * kRec : nullptr;
        if (!grad_plain_occ_on(coef[j].s.k)) {   // -no_occ: no term reaches the occlusions, +0.0 everywhere
            const hipError_t e = hipMemsetAsync(v.gp.o, 0, (size_t)n * 2 * v.h * v.w * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
        if (past && ssim)
            hipLaunchKernelGGL((table_loss_grad_plain_kernel<true, true>), v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j], r, (size_t)L * kRec);
        else if (past)
            hipLaunchKernelGGL((table_loss_grad_plain_kernel<true, false>), v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j], r, (size_t)L * kRec);
        else if (ssim)
            hipLaunchKernelGGL((table_loss_grad_plain_kernel<false, true>), v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j], r, (size_t)L * kRec);
        else
            hipLaunchKernelGGL((table_loss_grad_plain_kernel<false, false>), v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j], r, (size_t)L * kRec);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f
