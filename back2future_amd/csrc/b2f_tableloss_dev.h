// What the kernel files of the table loss share (b2f_tableloss.hip: test.lua:266-297; b2f_tableloss_ft.hip: the fine-tuning terms of
// README.md:89-102; b2f_tableloss_ssim.hip: the SSIM + L1 sums; b2f_tableloss_grad.hip: the gradient table of train.lua:428-468;
// b2f_tableloss_grad_ft.hip: that gradient with the fine-tuning criteria; b2f_tableloss_grad_ssim.hip: with the SSIM + L1 term).  Device side: how a thread loads and stores its pixels of a row, where the planes of a level lie, the
// five-point cross and the first-order smoothness of the two gradient kernels.  Host side: the one walk over the levels that every
// launcher makes (loss_levels).  For .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "b2f_tableloss_grad.h"

namespace b2f {

constexpr int kLossPx = 4;          // consecutive pixels of a row per thread: one 16-byte load per plane and row
constexpr int kLossThreads = 256;   // of a block of every kernel of the table loss

// n (1..4) samples of a row at p: one 16-byte load where the address allows -- rows of odd w are not aligned --, scalar loads
// otherwise; v[n..] is left alone
__device__ __forceinline__ void load_px(const float *p, int n, float *v)
{
    if (n == kLossPx && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kLossPx; ++k)
        if (k < n) v[k] = p[k];
}

// n (1..4) samples of a row to p: one 16-byte store where the address allows, scalar stores otherwise
__device__ __forceinline__ void store_px(float *p, int n, const float *v)
{
    if (n == kLossPx && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int k = 0; k < kLossPx; ++k)
        if (k < n) p[k] = v[k];
}

// the planes of one level: image 0; image b lies 2 hw (f, p, o), 3 hw (iw1, iw3) or ref_stride (ref) samples further
struct LevelPtrs {
    const float *f, *p, *o, *iw1, *iw3, *ref;
    size_t ref_stride;
};

// the gradient planes of one level: image 0; image b lies as far on as in the table
struct GradPtrs {
    float *f, *p, *o, *iw1, *iw3;
};

// where a group lies: its first pixel, how many of its pixels are in the row, which neighbours exist
struct Group {
    size_t i0;
    int x0, n, w;
    bool u1, u2, d1, d2;   // the rows y - 1, y - 2, y + 1, y + 2 exist
};

__device__ __forceinline__ Group group_at(int y, int x0, int h, int w)
{
    Group g;
    g.x0 = x0; g.w = w;
    g.n = w - x0 < kLossPx ? w - x0 : kLossPx;
    g.i0 = (size_t)y * w + x0;
    g.u1 = y > 0; g.u2 = y > 1; g.d1 = y + 1 < h; g.d2 = y + 2 < h;
    return g;
}

// the five-point cross of a group in one plane: cur[1..4] the group (loaded here unless the caller holds it: Centre = false), cur[0] /
// cur[5] the pixel left / right of it, up / low the rows above / below; what does not exist is 0 and is not read by a term.  Every
// index lies in the plane (k < n, x0 > 0, x0 + 4 < w, u1, d1).
template <bool Centre>
__device__ __forceinline__ void load_cross(const float *pl, const Group &g, float *cur, float *up, float *low)
{
#pragma unroll
    for (int k = 0; k < kLossPx; ++k) {
        up[k] = low[k] = 0.0f;
        if (Centre) cur[k + 1] = 0.0f;
    }
    cur[0] = cur[kLossPx + 1] = 0.0f;
    if (Centre) load_px(pl + g.i0, g.n, cur + 1);
    if (g.x0 > 0) cur[0] = pl[g.i0 - 1];
    if (g.x0 + kLossPx < g.w) cur[kLossPx + 1] = pl[g.i0 + kLossPx];
    if (g.u1) load_px(pl + g.i0 - g.w, g.n, up);
    if (g.d1) load_px(pl + g.i0 + g.w, g.n, low);
}

// S of the group's four pixels in one plane from its five-point cross; wx[i]: the pair of columns x0 - 1 + i and x0 + i, wyc / wyu: the
// pairs with the row below / above.  a[i] serves the pixel right of the pair as a(x - 1, y) and the pixel left of it as a(x, y).
template <bool Quad>
__device__ __forceinline__ void smooth4(const float *cur, const float *up, const float *low, const Group &g, const double *wx, const double *wyc,
                                        const double *wyu, double *S)
{
    double a[kLossPx + 1];
#pragma unroll
    for (int i = 0; i <= kLossPx; ++i) a[i] = grad_edge<Quad>(g.x0 - 1 + i >= 0 && g.x0 + i < g.w, cur[i], cur[i + 1], wx[i]);
#pragma unroll
    for (int k = 0; k < kLossPx; ++k)
        S[k] = grad_s(a[k + 1], a[k], grad_edge<Quad>(g.d1, cur[k + 1], low[k], wyc[k]), grad_edge<Quad>(g.u1, up[k], cur[k + 1], wyu[k]));
}

// ---- host side: the walk over the levels ----
// what a launcher needs of level j: its size, kd = flow_scale / 2^j, its planes (lp.ref: R_0 = ref, R_j at pyr + pyr_off), its
// gradient planes where there is a gradient table, and the grid of its kernel
struct LossLevel {
    int h, w;
    float kd;
    LevelPtrs lp;
    GradPtrs gp;
    size_t pyr_off;
    dim3 grid;
};

// floats of R_j (n x 3 x h x w) in the workspace: every level 16-byte aligned
inline size_t loss_level_floats(int n, int h, int w) { return ((size_t)n * 3 * h * w + 3) & ~(size_t)3; }

// The walk without a table, for the pyramid's launcher: checks what every launcher checks of the shape, the reference image and the
// workspace, and fills h, w, lp.ref, lp.ref_stride and pyr_off of lv[0 .. L).  false: an argument is refused.
inline bool loss_levels(int L, int n, int H, int W, const float *ref, size_t ref_stride, const float *pyr, LossLevel *lv)
{
    if (n <= 0 || n > 65535 || L < 1 || L > kLossMaxLevels || H <= 0 || W <= 0 || (size_t)H * W >= (size_t)kPhotoMaxPixels || H % (1 << (L - 1)) ||
        W % (1 << (L - 1)) || !ref || (L > 1 && !pyr) || ref_stride < (size_t)3 * H * W)
        return false;
    size_t off = 0;
    for (int j = 0; j < L; ++j) {
        LossLevel &v = lv[j];
        v = LossLevel{};
        v.h = H >> j; v.w = W >> j;
        v.pyr_off = off;
        v.lp.ref = j ? pyr + off : ref;
        v.lp.ref_stride = j ? (size_t)3 * v.h * v.w : ref_stride;
        if (j) off += loss_level_floats(n, v.h, v.w);
    }
    return true;
}

// The walk of a kernel's launcher: the same, and the planes of the table (L x (4 | 5) tensors, none null), of the gradient table where
// there is one (grad, else nullptr), kd and the grid.  The grid is capped as for the photometric record: about eight blocks per CU
// over the whole call and not too many per image (a full-HD image alone wraps the kernel's loop), so that few blocks add to a record.
inline bool loss_levels(const float *const *table, float *const *grad, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride,
                        const float *pyr, double flow_scale, LossLevel *lv)
{
    if (!table || !loss_levels(L, n, H, W, ref, ref_stride, pyr, lv)) return false;
    const int per = past ? 5 : 4;
    for (int i = 0; i < L * per; ++i)
        if (!table[i] || (grad && !grad[i])) return false;
    const size_t cap = std::min<size_t>(1024, std::max<size_t>(8, 2048 / (size_t)n));
    for (int j = 0; j < L; ++j) {
        LossLevel &v = lv[j];
        const float *const *t = table + (size_t)j * per;
        const LevelPtrs lp = {t[0], past ? t[1] : nullptr, t[per - 3], t[per - 2], t[per - 1], v.lp.ref, v.lp.ref_stride};
        v.lp = lp;
        if (grad) {
            float *const *g = grad + (size_t)j * per;
            const GradPtrs gp = {g[0], past ? g[1] : nullptr, g[per - 3], g[per - 2], g[per - 1]};
            v.gp = gp;
        }
        v.kd = (float)(flow_scale / (double)(1 << j));
        const size_t groups = (((size_t)v.w + kLossPx - 1) / kLossPx) * (size_t)v.h, blocks = (groups + kLossThreads - 1) / kLossThreads;
        v.grid = dim3((unsigned)std::min(blocks, cap), (unsigned)n);
    }
    return true;
}

// The launcher of the kernels that add their own words to records of record_words words the records' launch has zeroed (the
// fine-tuning terms, the SSIM + L1 sums, the sums without occlusion masking): one launch per level, of kernel_true on a table with past
// flows and of kernel_false on one without.  Both are (LevelPtrs, h, w, kd, the level's record of image 0, words from one image to the next).
template <class Kernel>
hipError_t launch_terms(Kernel kernel_true, Kernel kernel_false, int record_words, const float *const *table, int L, bool past, int n, int H, int W,
                        const float *ref, size_t ref_stride, const float *pyr, double flow_scale, unsigned long long *loss, hipStream_t s)
{
    LossLevel lv[kLossMaxLevels];
    if (!loss || !loss_levels(table, nullptr, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, lv)) return hipErrorInvalidValue;
    const Kernel kernel = past ? kernel_true : kernel_false;
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        hipLaunchKernelGGL(kernel, v.grid, dim3(kLossThreads), 0, s, v.lp, v.h, v.w, v.kd, loss + (size_t)j * record_words,
                           (size_t)L * record_words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f
