// The occlusion-aware SSIM + L1 photometric term (opts.lua:62: -pme_criterion OSSIM | OSSIML1; criterions/OSSIML1Criterion.lua:47-163)
// on the device: words 16 .. 25 of the records of B2F_LOSS_SSIM_WORDS integers per image and level, beside words 0 .. 15, which
// table_loss_kernel of b2f_tableloss.hip (test.lua:266-297) writes unchanged into the wider record first.  Two stages:
//   table_loss_range_kernel: the minimum and maximum of an image's nine planes at a level (R_j and both warped images), 16-byte
//     loads where the address allows, a wave reduction, the waves of a block through LDS, then one integer atomicMax per block and
//     word on the order-preserving encoding of the float (b2f_tableloss_ssim.h: ssim_enc) -- exact, whatever the order.
//     table_loss_range_finish_kernel decodes them into words 24 / 25 and writes the range the pixels use into words 22 / 23: the
//     image's own, the batch's (combined here, on the device) or the caller's.  Both kernels have a second instantiation for the records
//     of b2f_tableloss_plain.hip: other words, and the occlusions and the past flow as further planes (MSSIML1Criterion.lua:63-68).
//   table_loss_ssim_kernel has the structure of table_loss_ft_kernel -- a thread covers four consecutive pixels of a row, the rows
//     above and below come through the cache (DESIGN.md 7.9 says why no LDS tile), counters in registers, the same block reduction,
//     at most one 64-bit atomicAdd per non-zero word per block, the same capped grid -- on the 3 x 3 window with replication: per
//     plane the column sums of the six columns a group's four windows span are computed once, and the reference's window sums once
//     for both directions.
// The per-pixel functions are those of b2f_tableloss_ssim.h, which the host entry (b2f_table_loss_ssim_host) shares.
#include "b2f_ctx.h"
#include "b2f_tableloss_ssim_dev.h"

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px)
constexpr int kThreads = kLossThreads;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kRec = B2F_LOSS_SSIM_WORDS;
constexpr int kFirst = B2F_LOSS_SSIM_Q30;   // the first word table_loss_ssim_kernel adds to
constexpr int kWords = B2F_LOSS_SSIM_RANGE_USED - kFirst;
constexpr int kCols = kSsimCols;            // the columns x0 - 1 .. x0 + 4 of a group's windows (b2f_tableloss_ssim_dev.h)

// the encoded minimum (lo) and maximum (hi) of p[0 .. len) but its NaNs, over the threads of a block's stride
__device__ __forceinline__ void range_of(const float *p, size_t len, size_t t0, size_t stride, unsigned &lo, unsigned &hi)
{
    auto take = [&](float v) {
        if (v == v) {
            const unsigned e = ssim_enc(v);
            lo = e < lo ? e : lo;
            hi = e > hi ? e : hi;
        }
    };
    const size_t mis = ((uintptr_t)p & 15) / sizeof(float);           // p is a float pointer: 0 .. 3 samples past a 16-byte boundary
    const size_t lead = (kPx - mis) % kPx, head = lead < len ? lead : len;   // scalar samples up to the first aligned one
    const size_t quads = (len - head) / kPx, tail = head + quads * kPx;
    for (size_t i = t0; i < head; i += stride) take(p[i]);
    for (size_t q = t0; q < quads; q += stride) {
        const float4 v = *reinterpret_cast<const float4 *>(p + head + q * kPx);
        take(v.x); take(v.y); take(v.z); take(v.w);
    }
    for (size_t i = tail + t0; i < len; i += stride) take(p[i]);
}

// where the two pairs of a record lie and how long it is: the SSIM records, or (Plain) those of the terms without occlusion masking
template <bool Plain>
struct RangeRec {
    static constexpr int kOwn = Plain ? B2F_LOSS_PLAIN_RANGE_OWN : B2F_LOSS_SSIM_RANGE_OWN;
    static constexpr int kUsed = Plain ? B2F_LOSS_PLAIN_RANGE_USED : B2F_LOSS_SSIM_RANGE_USED;
    static constexpr int kWords = Plain ? B2F_LOSS_PLAIN_WORDS : B2F_LOSS_SSIM_WORDS;
};

// Image blockIdx.y of one level: words OWN_MIN / OWN_MAX of its record (zero before) gather the complement of the encoded minimum and
// the encoded maximum, so that zero is the identity of both and one atomicMax serves each.  Plain: the range of
// MSSIML1Criterion.lua:63-68, whose loop starts at input[2]: the two occlusion planes and, where lp.p is not null, the two planes of
// the past flow are part of it.
template <bool Plain>
__global__ void __launch_bounds__(kThreads) table_loss_range_kernel(LevelPtrs lp, int h, int w, unsigned long long *loss, size_t rec_stride)
{
    constexpr int kOwn = RangeRec<Plain>::kOwn;
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const float *seg[3] = {lp.ref + b * lp.ref_stride, lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};   // three planes each, contiguous
    unsigned lo = 0xffffffffu, hi = 0u;
    const size_t t0 = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
#pragma unroll
    for (int k = 0; k < 3; ++k) range_of(seg[k], 3 * hw, t0, stride, lo, hi);
    if (Plain) {
        range_of(lp.o + b * 2 * hw, 2 * hw, t0, stride, lo, hi);
        if (lp.p) range_of(lp.p + b * 2 * hw, 2 * hw, t0, stride, lo, hi);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned l2 = __shfl_down(lo, off, kWave), h2 = __shfl_down(hi, off, kWave);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    __shared__ unsigned part[kWaves][2];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
        part[wave][0] = lo;
        part[wave][1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kWaves; ++k) {
            lo = part[k][0] < lo ? part[k][0] : lo;
            hi = part[k][1] > hi ? part[k][1] : hi;
        }
        unsigned long long *rec = loss + b * rec_stride;
        if (~lo) atomicMax(rec + kOwn, (unsigned long long)(~lo));
        if (hi) atomicMax(rec + kOwn + 1, (unsigned long long)hi);
    }
}

struct GivenRanges {
    float r[kLossMaxLevels][2];
};

// Level blockIdx.x of all n images: words RANGE_OWN of every record from what table_loss_range_kernel gathered to the float bits of
// the image's own minimum and maximum, words RANGE_USED to the float bits of the range of `mode`.  One block: the batch's range is
// complete before the first record is rewritten.
template <bool Plain>
__global__ void __launch_bounds__(kThreads) table_loss_range_finish_kernel(unsigned long long *loss, int n, int L, int mode, GivenRanges given)
{
    constexpr int kOwn = RangeRec<Plain>::kOwn, kUsed = RangeRec<Plain>::kUsed, kRec = RangeRec<Plain>::kWords;
    const int j = blockIdx.x;
    __shared__ unsigned all[2];
    if (threadIdx.x == 0) {
        all[0] = 0xffffffffu;
        all[1] = 0u;
    }
    __syncthreads();
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int b = threadIdx.x; b < n; b += kThreads) {
        const unsigned long long *rec = loss + ((size_t)b * L + j) * kRec;
        const unsigned l2 = ~(unsigned)rec[kOwn], h2 = (unsigned)rec[kOwn + 1];
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    atomicMin(&all[0], lo);
    atomicMax(&all[1], hi);
    __syncthreads();
    for (int b = threadIdx.x; b < n; b += kThreads) {
        unsigned long long *rec = loss + ((size_t)b * L + j) * kRec;
        const unsigned own_lo = ~(unsigned)rec[kOwn], own_hi = (unsigned)rec[kOwn + 1];
        unsigned mn = ssim_dec_bits(own_lo), mx = ssim_dec_bits(own_hi);
        rec[kOwn] = mn;
        rec[kOwn + 1] = mx;
        if (mode == B2F_SSIM_RANGE_BATCH) {
            mn = ssim_dec_bits(all[0]);
            mx = ssim_dec_bits(all[1]);
        } else if (mode == B2F_SSIM_RANGE_GIVEN) {
            mn = __float_as_uint(given.r[j][0]);
            mx = __float_as_uint(given.r[j][1]);
        }
        rec[kUsed] = mn;
        rec[kUsed + 1] = mx;
    }
}

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  loss: the record of image 0 at this
// level, image b lies `rec_stride` words further; words kFirst .. kFirst + kWords are zero before, words RANGE_USED hold the range.
template <bool Past>
__global__ void __launch_bounds__(kThreads) table_loss_ssim_kernel(LevelPtrs lp, int h, int w, float kd, unsigned long long *loss, size_t rec_stride)
{
#pragma clang fp contract(off)
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    const unsigned long long *own = loss + b * rec_stride;
    const SsimRange rg = ssim_range(__uint_as_float((unsigned)own[B2F_LOSS_SSIM_RANGE_USED]), __uint_as_float((unsigned)own[B2F_LOSS_SSIM_RANGE_USED + 1]));
    const float *fl[2] = {(Past ? lp.p : lp.f) + b * 2 * hw, lp.f + b * 2 * hw};   // the flow of the direction (OSSIML1Criterion.lua:131-132)
    const float *occ = lp.o + b * 2 * hw;
    const float *ref = lp.ref + b * lp.ref_stride;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    unsigned long long ssim[2] = {0, 0}, l1n[2] = {0, 0};
    unsigned nonf[2] = {0, 0};
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const size_t up = y > 0 ? (size_t)w : 0, down = y + 1 < h ? (size_t)w : 0;   // the clamped rows above and below
        const bool before = x0 > 0, more = x0 + kPx < w;
        // which pixel-directions count in PHOTO_INSIDE, and their weights
        bool counted[2][kPx];
        float wt[2][kPx];
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
                float fv[2][kPx], wv[3][kPx];
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
                for (int k = 0; k < kPx; ++k) wt[d][k] = 0.0f;
                load_px(occ + (size_t)(1 - d) * hw + i0, n, wt[d]);
#pragma unroll
                for (int k = 0; k < kPx; ++k) {
                    const bool live = k < n;
                    // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not counted
                    const WarpTaps tp = warp_taps(fv[0][k], fv[1][k], d == 0 ? -kd : kd, live ? x0 + k : x0, y, w, h);
                    const float w3[3] = {wv[0][k], wv[1][k], wv[2][k]}, r3[3] = {rv[0][k], rv[1][k], rv[2][k]};
                    counted[d][k] = live && photo_pixel(tp, w3, r3, true, wt[d][k]).inside != 0u;
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
                const PixelSsim ps = ssim_pixel(S[d][k], B[d][k], counted[d][k], rg.ok, wt[d][k]);
                ssim[d] += ps.ssim;
                l1n[d] += ps.l1n;
                nonf[d] += ps.nonfinite;
            }
    }
    // the words of this thread, then of its wave
    unsigned long long rec[kWords];
    rec[B2F_LOSS_SSIM_Q30 - kFirst] = ssim[0];          rec[B2F_LOSS_SSIM_Q30 - kFirst + 1] = ssim[1];
    rec[B2F_LOSS_SSIM_L1N_Q30 - kFirst] = l1n[0];       rec[B2F_LOSS_SSIM_L1N_Q30 - kFirst + 1] = l1n[1];
    rec[B2F_LOSS_SSIM_NONFINITE - kFirst] = nonf[0];    rec[B2F_LOSS_SSIM_NONFINITE - kFirst + 1] = nonf[1];
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

hipError_t launch_table_loss_range(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride, const float *pyr,
                                   int range_mode, const float *ranges, unsigned long long *loss, hipStream_t s, bool plain)
{
    const int words = plain ? B2F_LOSS_PLAIN_WORDS : kRec;
    LossLevel lv[kLossMaxLevels];
    if (!loss || range_mode < B2F_SSIM_RANGE_BATCH || range_mode > B2F_SSIM_RANGE_GIVEN || (range_mode == B2F_SSIM_RANGE_GIVEN && !ranges) ||
        !loss_levels(table, nullptr, L, past, n, H, W, ref, ref_stride, pyr, 1.0, lv))
        return hipErrorInvalidValue;
    GivenRanges given = {};
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        if (range_mode == B2F_SSIM_RANGE_GIVEN) {
            given.r[j][0] = ranges[2 * j];
            given.r[j][1] = ranges[2 * j + 1];
        }
        if (plain)
            hipLaunchKernelGGL(table_loss_range_kernel<true>, v.grid, dim3(kThreads), 0, s, v.lp, v.h, v.w, loss + (size_t)j * words, (size_t)L * words);
        else
            hipLaunchKernelGGL(table_loss_range_kernel<false>, v.grid, dim3(kThreads), 0, s, v.lp, v.h, v.w, loss + (size_t)j * words, (size_t)L * words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (plain)
        hipLaunchKernelGGL(table_loss_range_finish_kernel<true>, dim3((unsigned)L), dim3(kThreads), 0, s, loss, n, L, range_mode, given);
    else
        hipLaunchKernelGGL(table_loss_range_finish_kernel<false>, dim3((unsigned)L), dim3(kThreads), 0, s, loss, n, L, range_mode, given);
    return hipGetLastError();
}

hipError_t launch_table_loss_ssim_terms(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride,
                                        const float *pyr, double flow_scale, unsigned long long *loss, hipStream_t s)
{
    return launch_terms(table_loss_ssim_kernel<true>, table_loss_ssim_kernel<false>, kRec, table, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, loss, s);
}

}  // namespace b2f
