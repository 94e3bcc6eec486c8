// The gradient of the -optimize pme objective with respect to the output table on the device: `gradOutputs` of train.lua:428-468, the
// 4 (Hard) or 5 (Soft) tensors of every level.  table_loss_grad_kernel has the structure of table_loss_ft_kernel (b2f_tableloss_ft.hip)
// -- one launch per level over the same capped (blocks, n) grid, a thread covers consecutive pixels of a row, 16-byte loads where
// the address allows, the rows above and below through the cache -- but it reduces nothing: a pure streaming
// kernel without LDS or atomics that reads the five-point cross of f, p, o and R and the centre of the six warped planes and writes
// its pixels of the 10 (Hard) or 12 (Soft) gradient planes, one 16-byte store per plane where the address allows.  A group needs the
// contrast weight wx at five pairs of columns and wy at two rows of four columns: 13 exponentials per four pixels, each computed once
// and shared by the six smoothed planes.  The per-element functions are those of b2f_tableloss_grad.h, which the host entry
// (b2f_table_loss_grad_host) shares, so both give the same bits.
#include "b2f_ctx.h"
#include "b2f_tableloss_grad.h"
#include "b2f_tableloss_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px, store_px)
constexpr int kThreads = kLossThreads;

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.
template <bool Past>
__global__ void __launch_bounds__(kThreads) table_loss_grad_kernel(LevelPtrs lp, GradPtrs gp, int h, int w, float kd, GradCoef k)
{
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const float *R = lp.ref + b * lp.ref_stride;
    const float *f = lp.f + b * 2 * hw, *p = Past ? lp.p + b * 2 * hw : nullptr, *o = lp.o + b * 2 * hw;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    float *gf = gp.f + b * 2 * hw, *gpp = Past ? gp.p + b * 2 * hw : nullptr, *go = gp.o + b * 2 * hw;
    float *giw[2] = {gp.iw1 + b * 3 * hw, gp.iw3 + b * 3 * hw};
    const bool on_s = (k.on & kGradSmooth) != 0, on_cv = Past && (k.on & kGradConstVel) != 0, on_p = (k.on & kGradPhoto) != 0,
               on_so = (k.on & kGradSmoothOcc) != 0;
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const Group g = group_at(y, x0, h, w);
        const int n = g.n;
        const size_t i0 = g.i0;
        // the reference image: its centre for the photometric term, its cross for the 13 contrast weights
        float rc[3][kPx + 2], ru[3][kPx], rl[3][kPx];
        double wx[kPx + 1], wyc[kPx], wyu[kPx];
        if (on_s || on_so) {
#pragma unroll
            for (int c = 0; c < 3; ++c) load_cross<true>(R + (size_t)c * hw, g, rc[c], ru[c], rl[c]);
#pragma unroll
            for (int i = 0; i <= kPx; ++i)
                wx[i] = grad_weight(x0 - 1 + i >= 0 && x0 + i < w, rc[0][i], rc[0][i + 1], rc[1][i], rc[1][i + 1], rc[2][i], rc[2][i + 1]);
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                wyc[q] = grad_weight(g.d1, rc[0][q + 1], rl[0][q], rc[1][q + 1], rl[1][q], rc[2][q + 1], rl[2][q]);
                wyu[q] = grad_weight(g.u1, ru[0][q], rc[0][q + 1], ru[1][q], rc[1][q + 1], ru[2][q], rc[2][q + 1]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int q = 0; q < kPx; ++q) rc[c][q + 1] = 0.0f;
                load_px(R + (size_t)c * hw + i0, n, rc[c] + 1);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) wx[q] = wyc[q] = wyu[q] = 1.0;
            wx[kPx] = 1.0;
        }
        // the centres of the flows and of the occlusions
        float fc[2][kPx + 2], pc[2][kPx + 2], oc[2][kPx + 2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int q = 0; q < kPx; ++q) fc[c][q + 1] = pc[c][q + 1] = oc[c][q + 1] = 0.0f;
            load_px(f + (size_t)c * hw + i0, n, fc[c] + 1);
            if (Past) load_px(p + (size_t)c * hw + i0, n, pc[c] + 1);
            load_px(o + (size_t)c * hw + i0, n, oc[c] + 1);
        }
        // the photometric term: G_iw_d, and PO for the occlusions (po[c][q] = PO_c: direction d fills channel 1 - d)
        double po[2][kPx];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            float wv[3][kPx], out[3][kPx];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int q = 0; q < kPx; ++q) wv[c][q] = out[c][q] = 0.0f;
                if (on_p) load_px(iw[d] + (size_t)c * hw + i0, n, wv[c]);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                po[1 - d][q] = 0.0;
                if (on_p) {
                    const bool pf = d == 0 && Past;   // OBCCriterion.lua:166-170
                    // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not stored
                    const WarpTaps tp = warp_taps(pf ? pc[0][q + 1] : fc[0][q + 1], pf ? pc[1][q + 1] : fc[1][q + 1], d == 0 ? -kd : kd, q < n ? x0 + q : x0,
                                                  y, w, h);
                    const float w3[3] = {wv[0][q], wv[1][q], wv[2][q]}, r3[3] = {rc[0][q + 1], rc[1][q + 1], rc[2][q + 1]};
                    float g3[3];
                    grad_photo(k, tp.inside, w3, r3, oc[1 - d][q + 1], &po[1 - d][q], g3);
                    out[0][q] = g3[0]; out[1][q] = g3[1]; out[2][q] = g3[2];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) store_px(giw[d] + (size_t)c * hw + i0, n, out[c]);
        }
        // the occlusions
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float up[kPx], low[kPx], out[kPx];
            double S[kPx] = {0.0, 0.0, 0.0, 0.0};
            if (on_so) {
                load_cross<false>(o + (size_t)c * hw, g, oc[c], up, low);
                smooth4<true>(oc[c], up, low, g, wx, wyc, wyu, S);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) out[q] = grad_occ(k, po[c][q], S[q], oc[1 - c][q + 1]);
            store_px(go + (size_t)c * hw + i0, n, out);
        }
        // the flows
        double cv[kPx][2];
#pragma unroll
        for (int q = 0; q < kPx; ++q) {
            cv[q][0] = cv[q][1] = 0.0;
            if (on_cv) grad_const_vel(fc[0][q + 1], fc[1][q + 1], pc[0][q + 1], pc[1][q + 1], cv[q]);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float up[kPx], low[kPx], out[kPx];
            double S[kPx] = {0.0, 0.0, 0.0, 0.0};
            if (on_s) {
                load_cross<false>(f + (size_t)c * hw, g, fc[c], up, low);
                smooth4<false>(fc[c], up, low, g, wx, wyc, wyu, S);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) out[q] = grad_flow(k, S[q], cv[q][c], Past, false);
            store_px(gf + (size_t)c * hw + i0, n, out);
            if (Past) {
                if (on_s) {
                    load_cross<false>(p + (size_t)c * hw, g, pc[c], up, low);
                    smooth4<false>(pc[c], up, low, g, wx, wyc, wyu, S);
                }
#pragma unroll
                for (int q = 0; q < kPx; ++q) out[q] = grad_flow(k, S[q], cv[q][c], true, true);
                store_px(gpp + (size_t)c * hw + i0, n, out);
            }
        }
    }
}

}  // namespace

hipError_t launch_table_loss_grad(const float *const *table, float *const *grad, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride,
                                  const float *pyr, double flow_scale, const GradCoef *coef, hipStream_t s)
{
    LossLevel lv[kLossMaxLevels];
    if (!grad || !coef || !loss_levels(table, grad, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, lv)) return hipErrorInvalidValue;
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        if (past)
            hipLaunchKernelGGL(table_loss_grad_kernel<true>, v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j]);
        else
            hipLaunchKernelGGL(table_loss_grad_kernel<false>, v.grid, dim3(kThreads), 0, s, v.lp, v.gp, v.h, v.w, v.kd, coef[j]);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f
