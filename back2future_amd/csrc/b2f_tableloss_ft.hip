// The fine-tuning objective of the Soft models (README.md:89-102: -smooth_second_order, -pme_criterion OBGCC) on the device: words
// 16 .. 23 of the records of B2F_LOSS_FT_WORDS integers per image and level, beside words 0 .. 15, which table_loss_kernel of
// b2f_tableloss.hip (test.lua:266-297) writes unchanged into the wider record first.  table_loss_ft_kernel has that kernel's structure -- a
// thread covers consecutive pixels of a row, 16-byte loads where the address allows, counters in registers, a wave reduction, the
// waves of a block through LDS, at most one 64-bit atomicAdd per non-zero word per block, the same capped grid -- on a wider
// stencil: the flows and the reference image at the five-point cross of criterions/SecondOrderSmoothnessCriterion.lua:45-58, the six
// warped planes and the reference at (x, x + 1, y + 1) for the forward differences of criterions/OBGCCriterion.lua:67-68,91-92.  The
// rows above and below come through the cache like the lower row of table_loss_kernel (DESIGN.md 7.9 says why no LDS tile).  The
// per-pixel functions are those of b2f_tableloss_ft.h, which the host entry (b2f_table_loss_ft_host) shares.
#include "b2f_ctx.h"
#include "b2f_tableloss_ft.h"
#include "b2f_tableloss_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px)
constexpr int kThreads = kLossThreads;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kFirst = B2F_LOSS_FT_SMOOTH2_FLOW_Q30;   // the first word this kernel writes
constexpr int kWords = B2F_LOSS_FT_WORDS - kFirst;

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  loss: the record of image 0 at this
// level, image b lies `rec_stride` words further; words kFirst .. are zero before.
template <bool Past>
__global__ void __launch_bounds__(kThreads) table_loss_ft_kernel(LevelPtrs lp, int h, int w, float kd, unsigned long long *loss, size_t rec_stride)
{
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    constexpr int kPl = 7;   // f0 f1 p0 p1 R0 R1 R2 (b2f_tableloss_ft.h: smooth2_pixel)
    const float *pl[kPl];
    pl[0] = lp.f + b * 2 * hw; pl[1] = pl[0] + hw;
    pl[2] = Past ? lp.p + b * 2 * hw : nullptr; pl[3] = Past ? pl[2] + hw : nullptr;
    pl[4] = lp.ref + b * lp.ref_stride; pl[5] = pl[4] + hw; pl[6] = pl[5] + hw;
    const float *occ = lp.o + b * 2 * hw;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    unsigned s2_nonf = 0, g_nonf = 0;
    unsigned long long s2_flow = 0, s2_past = 0, ogx[2] = {0, 0}, ogy[2] = {0, 0};
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const bool has_u = y > 0, has_d = y + 1 < h, before = x0 > 0, more = x0 + kPx < w;
        // cur[c][1..4] the group, cur[c][0] / cur[c][5] the pixel left / right of it, up / low the rows above / below: every index lies in
        // the plane (k < n, before, more, has_u, has_d)
        float cur[kPl][kPx + 2], up[kPl][kPx], low[kPl][kPx];
#pragma unroll
        for (int c = 0; c < kPl; ++c) {
#pragma unroll
            for (int k = 0; k < kPx; ++k) cur[c][k + 1] = up[c][k] = low[c][k] = 0.0f;
            cur[c][0] = cur[c][kPx + 1] = 0.0f;
            if (!Past && (c == 2 || c == 3)) continue;
            load_px(pl[c] + i0, n, cur[c] + 1);
            if (before) cur[c][0] = pl[c][i0 - 1];
            if (more) cur[c][kPx + 1] = pl[c][i0 + kPx];
            if (has_u) load_px(pl[c] + i0 - w, n, up[c]);
            if (has_d) load_px(pl[c] + i0 + w, n, low[c]);
        }
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const bool live = k < n;
            float v[kPl], vl[kPl], vr[kPl], vu[kPl], vd[kPl];
#pragma unroll
            for (int c = 0; c < kPl; ++c) {
                vl[c] = cur[c][k];
                v[c] = cur[c][k + 1];
                vr[c] = cur[c][k + 2];
                vu[c] = up[c][k];
                vd[c] = low[c][k];
            }
            const PixelSmooth2 s = smooth2_pixel(v, vl, vr, vu, vd, x0 + k > 0, x0 + k + 1 < w, has_u, has_d, Past);
            s2_flow += live ? s.flow : 0ull;
            s2_past += live ? s.past : 0ull;
            s2_nonf += live ? s.nonfinite : 0u;
        }
        float ov[2][kPx];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int k = 0; k < kPx; ++k) ov[c][k] = 0.0f;
            load_px(occ + (size_t)c * hw + i0, n, ov[c]);
        }
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            // wv[c][0..3] the group of the direction's warped image, wv[c][4] the pixel right of it, wl[c] the row below
            float wv[3][kPx + 1], wl[3][kPx];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < kPx; ++k) wv[c][k] = wl[c][k] = 0.0f;
                wv[c][kPx] = 0.0f;
                const float *q = iw[d] + (size_t)c * hw + i0;
                load_px(q, n, wv[c]);
                if (more) wv[c][kPx] = q[kPx];
                if (has_d) load_px(q + w, n, wl[c]);
            }
            const bool pf = d == 0 && Past;   // OBGCCriterion.lua:110-111
#pragma unroll
            for (int k = 0; k < kPx; ++k) {
                const bool live = k < n;
                // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not counted
                const WarpTaps tp = warp_taps(pf ? cur[2][k + 1] : cur[0][k + 1], pf ? cur[3][k + 1] : cur[1][k + 1], d == 0 ? -kd : kd, live ? x0 + k : x0,
                                              y, w, h);
                const float w3[3] = {wv[0][k], wv[1][k], wv[2][k]}, w3x[3] = {wv[0][k + 1], wv[1][k + 1], wv[2][k + 1]};
                const float w3y[3] = {wl[0][k], wl[1][k], wl[2][k]};
                const float r3[3] = {cur[4][k + 1], cur[5][k + 1], cur[6][k + 1]}, r3x[3] = {cur[4][k + 2], cur[5][k + 2], cur[6][k + 2]};
                const float r3y[3] = {low[4][k], low[5][k], low[6][k]};
                const float p = d == 0 ? ov[1][k] : ov[0][k];
                const PixelPhoto ph = photo_pixel(tp, w3, r3, true, p);
                const PixelGrad g = grad_pixel(w3, w3x, w3y, r3, r3x, r3y, x0 + k + 1 < w, has_d, live && ph.inside != 0u, p);
                ogx[d] += g.ogx;
                ogy[d] += g.ogy;
                g_nonf += g.nonfinite;
            }
        }
    }
    // the words of this thread, then of its wave
    unsigned long long rec[kWords];
    rec[B2F_LOSS_FT_SMOOTH2_FLOW_Q30 - kFirst] = s2_flow;
    rec[B2F_LOSS_FT_SMOOTH2_PAST_Q30 - kFirst] = s2_past;
    rec[B2F_LOSS_FT_PHOTO_OGX_Q30 - kFirst] = ogx[0];   rec[B2F_LOSS_FT_PHOTO_OGX_Q30 - kFirst + 1] = ogx[1];
    rec[B2F_LOSS_FT_PHOTO_OGY_Q30 - kFirst] = ogy[0];   rec[B2F_LOSS_FT_PHOTO_OGY_Q30 - kFirst + 1] = ogy[1];
    rec[B2F_LOSS_FT_SMOOTH2_NONFINITE - kFirst] = s2_nonf;
    rec[B2F_LOSS_FT_GRAD_NONFINITE - kFirst] = g_nonf;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < kWords; ++j) rec[j] += __shfl_down(rec[j], off, kWave);
    }
    __shared__ unsigned long long part[kWaves][kWords];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kWords; ++j) part[wave][j] = rec[j];
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        unsigned long long sum = 0;
        for (int wv_ = 0; wv_ < kWaves; ++wv_) sum += part[wv_][threadIdx.x];
        if (sum) atomicAdd(loss + b * rec_stride + kFirst + threadIdx.x, sum);
    }
}

}  // namespace

hipError_t launch_table_loss_ft_terms(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride,
                                      const float *pyr, double flow_scale, unsigned long long *loss, hipStream_t s)
{
    return launch_terms(table_loss_ft_kernel<true>, table_loss_ft_kernel<false>, B2F_LOSS_FT_WORDS, table, L, past, n, H, W, ref, ref_stride, pyr, flow_scale,
                        loss, s);
}

}  // namespace b2f
