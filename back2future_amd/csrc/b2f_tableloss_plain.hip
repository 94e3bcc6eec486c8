// The photometric terms without occlusion masking (opts.lua:62: -pme_criterion BCC | SSIM | SSIML1; criterions/MBCCriterion.lua:35-102,
// criterions/MSSIML1Criterion.lua:45-153) on the device: words 16 .. 25 of the records of B2F_LOSS_PLAIN_WORDS integers per image and
// level, beside words 0 .. 15, which table_loss_kernel of b2f_tableloss.hip (test.lua:266-297) writes unchanged into the wider record
// first, and words 26 .. 29, the ranges, which the Plain instantiations of the range kernels of b2f_tableloss_ssim.hip write
// (MSSIML1Criterion.lua:63-68: over the occlusions and the past flow as well).
//   table_loss_plain_kernel has the structure of table_loss_ssim_kernel -- a thread covers four consecutive pixels of a row, the rows
//     above and below come through the cache (DESIGN.md 7.9 says why no LDS tile), counters in registers, the same block reduction, at
//     most one 64-bit atomicAdd per non-zero word per block, the same capped grid, the channel loop rolled, the
//     reference's window sums once for both directions.  photo_pixel on the raw values decides PHOTO_INSIDE as for words 6 / 7 and
//     gives q(B1) and q(B2) of MBCCriterion with it; the window pass gives S and B of MSSIML1Criterion without an occlusion weight.
// The per-pixel functions are those of b2f_tableloss_plain.h, which the host entry (b2f_table_loss_plain_host) shares.
#include "b2f_ctx.h"
#include "b2f_tableloss_plain.h"
#include "b2f_tableloss_ssim_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px)
constexpr int kThreads = kLossThreads;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kRec = B2F_LOSS_PLAIN_WORDS;
constexpr int kFirst = B2F_LOSS_PLAIN_L1_Q30;   // the first word table_loss_plain_kernel adds to
constexpr int kWords = B2F_LOSS_PLAIN_RANGE_USED - kFirst;
constexpr int kCols = kSsimCols;                // the columns x0 - 1 .. x0 + 4 of a group's windows (b2f_tableloss_ssim_dev.h)

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  loss: the record of image 0 at this
// level, image b lies `rec_stride` words further; words kFirst .. kFirst + kWords are zero before, words RANGE_USED hold the range.
template <bool Past>
__global__ void __launch_bounds__(kThreads) table_loss_plain_kernel(LevelPtrs lp, int h, int w, float kd, unsigned long long *loss, size_t rec_stride)
{
#pragma clang fp contract(off)
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const unsigned long long *own = loss + b * rec_stride;
    const SsimRange rg = ssim_range(__uint_as_float((unsigned)own[B2F_LOSS_PLAIN_RANGE_USED]), __uint_as_float((unsigned)own[B2F_LOSS_PLAIN_RANGE_USED + 1]));
    const float *fl[2] = {(Past ? lp.p : lp.f) + b * 2 * hw, lp.f + b * 2 * hw};   // the flow of the direction (MBCCriterion.lua:73-81)
    const float *occ = lp.o + b * 2 * hw;
    const float *ref = lp.ref + b * lp.ref_stride;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    unsigned long long l1[2] = {0, 0}, sq[2] = {0, 0}, ssim[2] = {0, 0}, l1n[2] = {0, 0};
    unsigned nonf[2] = {0, 0};
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const size_t up = y > 0 ? (size_t)w : 0, down = y + 1 < h ? (size_t)w : 0;   // the clamped rows above and below
        const bool before = x0 > 0, more = x0 + kPx < w;
        // which pixel-directions count in PHOTO_INSIDE, with their q(B1) and q(B2) on the raw values; a pixel past the row's end counts
        // nowhere
        unsigned counted[2] = {0u, 0u};   // bit k of counted[d]: pixel k counts in direction d
        {
            float rv[3][kPx];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < kPx; ++k) rv[c][k] = 0.0f;
                load_px(ref + (size_t)c * hw + i0, n, rv[c]);
            }
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                float fv[2][kPx], wv[3][kPx], wt[kPx];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int k = 0; k < kPx; ++k) wv[c][k] = 0.0f;
                    load_px(iw[d] + (size_t)c * hw + i0, n, wv[c]);
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int k = 0; k < kPx; ++k) fv[c][k] = 0.0f;
                    load_px(fl[d] + (size_t)c * hw + i0, n, fv[c]);
                }
#pragma unroll
                for (int k = 0; k < kPx; ++k) wt[k] = 0.0f;
                load_px(occ + (size_t)(1 - d) * hw + i0, n, wt);   // the weight of words 6 .. 9: a NaN in it keeps the pixel out of PHOTO_INSIDE
#pragma unroll
                for (int k = 0; k < kPx; ++k) {
                    const bool live = k < n;
                    // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not counted
                    const WarpTaps tp = warp_taps(fv[0][k], fv[1][k], d == 0 ? -kd : kd, live ? x0 + k : x0, y, w, h);
                    const float w3[3] = {wv[0][k], wv[1][k], wv[2][k]}, r3[3] = {rv[0][k], rv[1][k], rv[2][k]};
                    const PixelPlainRaw pr = plain_raw(photo_pixel(tp, w3, r3, true, wt[k]));
                    if (live && pr.counted) {
                        counted[d] |= 1u << k;
                        l1[d] += pr.l1;
                        sq[d] += pr.sq;
                    }
                }
            }
        }
        double S[2][kPx], B[2][kPx];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int k = 0; k < kPx; ++k) S[d][k] = B[d][k] = 0.0;
        if (rg.ok) {
            // one channel at a time: unrolled, all three channels' rows stay live and the kernel drops to one wave per SIMD
#pragma unroll 1
            for (int c = 0; c < 3; ++c) {
                double ty[3][kCols], mu_y[kPx], gyy[kPx];
                load_rows(ref + (size_t)c * hw, i0, up, down, n, before, more, rg, ty);
                window4(ty, nullptr, mu_y);
                window4(ty, ty, gyy);
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    double tx[3][kCols], mu_x[kPx], gxx[kPx], gxy[kPx];
                    load_rows(iw[d] + (size_t)c * hw, i0, up, down, n, before, more, rg, tx);
                    window4(tx, nullptr, mu_x);
                    window4(tx, tx, gxx);
                    window4(tx, ty, gxy);
#pragma unroll
                    for (int k = 0; k < kPx; ++k) {
                        const double s = ssim_term(mu_x[k], mu_y[k], gxx[k], gyy[k], gxy[k]), e = loss_p1(tx[1][k + 1] - ty[1][k + 1]);
                        S[d][k] = c == 0 ? s : S[d][k] + s;
                        B[d][k] = c == 0 ? e : B[d][k] + e;
                    }
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int k = 0; k < kPx; ++k) {
                const PixelPlainSsim pp = plain_ssim((counted[d] >> k & 1u) != 0u, S[d][k], B[d][k], rg.ok);
                ssim[d] += pp.ssim;
                l1n[d] += pp.l1n;
                nonf[d] += pp.nonfinite;
            }
    }
    // the words of this thread, then of its wave
    unsigned long long rec[kWords];
    rec[B2F_LOSS_PLAIN_L1_Q30 - kFirst] = l1[0];                 rec[B2F_LOSS_PLAIN_L1_Q30 - kFirst + 1] = l1[1];
    rec[B2F_LOSS_PLAIN_SQ_Q30 - kFirst] = sq[0];                 rec[B2F_LOSS_PLAIN_SQ_Q30 - kFirst + 1] = sq[1];
    rec[B2F_LOSS_PLAIN_SSIM_Q30 - kFirst] = ssim[0];             rec[B2F_LOSS_PLAIN_SSIM_Q30 - kFirst + 1] = ssim[1];
    rec[B2F_LOSS_PLAIN_L1N_Q30 - kFirst] = l1n[0];               rec[B2F_LOSS_PLAIN_L1N_Q30 - kFirst + 1] = l1n[1];
    rec[B2F_LOSS_PLAIN_SSIM_NONFINITE - kFirst] = nonf[0];       rec[B2F_LOSS_PLAIN_SSIM_NONFINITE - kFirst + 1] = nonf[1];
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

hipError_t launch_table_loss_plain_terms(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride,
                                         const float *pyr, double flow_scale, unsigned long long *loss, hipStream_t s)
{
    return launch_terms(table_loss_plain_kernel<true>, table_loss_plain_kernel<false>, kRec, table, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, loss, s);
}

}  // namespace b2f
