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
constexpr int kThreads = 256;

// the gradient planes of one level: image 0; image b lies as far on as in the table
struct GradPtrs {
    float *f, *p, *o, *iw1, *iw3;
};

// the cross of a group in one plane: cur[1..4] the group (loaded here unless the caller holds it: Centre = false), cur[0] / cur[5] the
// pixel left / right of it, up / low the rows above / below; what does not exist is 0 and is not read by a term.  Every index lies in
// the plane (k < n, before, more, has_u, has_d).
template <bool Centre>
__device__ __forceinline__ void load_cross(const float *pl, size_t i0, int n, int w, bool before, bool more, bool has_u, bool has_d, float *cur, float *up,
                                           float *low)
{
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
        up[k] = low[k] = 0.0f;
        if (Centre) cur[k + 1] = 0.0f;
    }
    cur[0] = cur[kPx + 1] = 0.0f;
    if (Centre) load_px(pl + i0, n, cur + 1);
    if (before) cur[0] = pl[i0 - 1];
    if (more) cur[kPx + 1] = pl[i0 + kPx];
    if (has_u) load_px(pl + i0 - w, n, up);
    if (has_d) load_px(pl + i0 + w, n, low);
}

// S of the group's four pixels in one plane; wx[i]: the pair of columns x0 - 1 + i and x0 + i, wyc / wyu: the pairs with the row below
// / above.  a[i] serves the pixel right of the pair as a(x - 1, y) and the pixel left of it as a(x, y).
template <bool Quad>
__device__ __forceinline__ void smooth4(const float *cur, const float *up, const float *low, int x0, int w, bool has_u, bool has_d, const double *wx,
                                        const double *wyc, const double *wyu, double *S)
{
    double a[kPx + 1];
#pragma unroll
    for (int i = 0; i <= kPx; ++i) a[i] = grad_edge<Quad>(x0 - 1 + i >= 0 && x0 + i < w, cur[i], cur[i + 1], wx[i]);
#pragma unroll
    for (int k = 0; k < kPx; ++k)
        S[k] = grad_s(a[k + 1], a[k], grad_edge<Quad>(has_d, cur[k + 1], low[k], wyc[k]), grad_edge<Quad>(has_u, up[k], cur[k + 1], wyu[k]));
}

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
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const bool has_u = y > 0, has_d = y + 1 < h, before = x0 > 0, more = x0 + kPx < w;
        // the reference image: its centre for the photometric term, its cross for the 13 contrast weights
        float rc[3][kPx + 2], ru[3][kPx], rl[3][kPx];
        double wx[kPx + 1], wyc[kPx], wyu[kPx];
        if (on_s || on_so) {
#pragma unroll
            for (int c = 0; c < 3; ++c) load_cross<true>(R + (size_t)c * hw, i0, n, w, before, more, has_u, has_d, rc[c], ru[c], rl[c]);
#pragma unroll
            for (int i = 0; i <= kPx; ++i)
                wx[i] = grad_weight(x0 - 1 + i >= 0 && x0 + i < w, rc[0][i], rc[0][i + 1], rc[1][i], rc[1][i + 1], rc[2][i], rc[2][i + 1]);
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                wyc[q] = grad_weight(has_d, rc[0][q + 1], rl[0][q], rc[1][q + 1], rl[1][q], rc[2][q + 1], rl[2][q]);
                wyu[q] = grad_weight(has_u, ru[0][q], rc[0][q + 1], ru[1][q], rc[1][q + 1], ru[2][q], rc[2][q + 1]);
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
                load_cross<false>(o + (size_t)c * hw, i0, n, w, before, more, has_u, has_d, oc[c], up, low);
                smooth4<true>(oc[c], up, low, x0, w, has_u, has_d, wx, wyc, wyu, S);
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
                load_cross<false>(f + (size_t)c * hw, i0, n, w, before, more, has_u, has_d, fc[c], up, low);
                smooth4<false>(fc[c], up, low, x0, w, has_u, has_d, wx, wyc, wyu, S);
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) out[q] = grad_flow(k, S[q], cv[q][c], Past, false);
            store_px(gf + (size_t)c * hw + i0, n, out);
            if (Past) {
                if (on_s) {
                    load_cross<false>(p + (size_t)c * hw, i0, n, w, before, more, has_u, has_d, pc[c], up, low);
                    smooth4<false>(pc[c], up, low, x0, w, has_u, has_d, wx, wyc, wyu, S);
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
    if (n <= 0 || n > 65535 || L < 1 || L > kLossMaxLevels || H <= 0 || W <= 0 || (size_t)H * W >= (size_t)kPhotoMaxPixels || H % (1 << (L - 1)) ||
        W % (1 << (L - 1)) || !table || !grad || !ref || !coef || (L > 1 && !pyr) || ref_stride < (size_t)3 * H * W)
        return hipErrorInvalidValue;
    const int per = past ? 5 : 4;
    for (int i = 0; i < L * per; ++i)
        if (!table[i] || !grad[i]) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    const float *R = ref;
    size_t R_stride = ref_stride;
    for (int j = 0; j < L; ++j) {
        const int h = H >> j, w = W >> j;
        const size_t hw = (size_t)h * w;
        if (j > 0) {   // where launch_table_loss / launch_table_loss_pyramid laid R_j
            R = pyr;
            R_stride = 3 * hw;
            pyr += ((size_t)n * 3 * hw + 3) & ~(size_t)3;
        }
        const float *const *t = table + (size_t)j * per;
        float *const *g = grad + (size_t)j * per;
        const LevelPtrs lp = {t[0], past ? t[1] : nullptr, t[per - 3], t[per - 2], t[per - 1], R, R_stride};
        const GradPtrs gp = {g[0], past ? g[1] : nullptr, g[per - 3], g[per - 2], g[per - 1]};
        const size_t groups = (((size_t)w + kPx - 1) / kPx) * (size_t)h, blocks = (groups + kThreads - 1) / kThreads;
        // the capped grid of launch_table_loss: about eight blocks per CU over the whole call, at most 1024 per image
        const size_t cap = std::min<size_t>(1024, std::max<size_t>(8, 2048 / (size_t)n));
        const dim3 grid((unsigned)std::min(blocks, cap), (unsigned)n);
        const float kd = (float)(flow_scale / (double)(1 << j));
        if (past)
            hipLaunchKernelGGL(table_loss_grad_kernel<true>, grid, dim3(kThreads), 0, s, lp, gp, h, w, kd, coef[j]);
        else
            hipLaunchKernelGGL(table_loss_grad_kernel<false>, grid, dim3(kThreads), 0, s, lp, gp, h, w, kd, coef[j]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f
