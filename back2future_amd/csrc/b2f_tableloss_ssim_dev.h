// The 3 x 3 window with replication on the device, shared by table_loss_ssim_kernel (b2f_tableloss_ssim.hip) and
// table_loss_grad_ssim_kernel (b2f_tableloss_grad_ssim.hip): a thread covers four consecutive pixels of a row, loads the three clamped
// rows of a plane over the six columns its four windows span, normalised, and forms the column sums once.  For .hip files only.
#pragma once
#include "b2f_tableloss_ssim.h"
#include "b2f_tableloss_dev.h"

namespace b2f {

constexpr int kSsimCols = kLossPx + 2;   // the columns x0 - 1 .. x0 + 4 of a group's windows

// The columns x0 - 1 .. x0 + 4 of one row of a plane, clamped to the row (replication), normalised: p points at the group's first pixel,
// n of its pixels are in the row.  Every index lies in the row (k < n, before, more).
__device__ __forceinline__ void load_row(const float *p, int n, bool before, bool more, const SsimRange &rg, double *t)
{
    float v[kSsimCols];
#pragma unroll
    for (int k = 0; k < kSsimCols; ++k) v[k] = 0.0f;
    load_px(p, n, v + 1);
    v[0] = before ? p[-1] : v[1];
#pragma unroll
    for (int k = 1; k < kLossPx; ++k) v[k + 1] = k < n ? v[k + 1] : v[k];   // past the row's end: its last pixel
    v[kLossPx + 1] = more ? p[kLossPx] : v[kLossPx];
#pragma unroll
    for (int k = 0; k < kSsimCols; ++k) t[k] = ssim_norm(v[k], rg);
}

// the three clamped rows of a group in one plane
__device__ __forceinline__ void load_rows(const float *pl, size_t i0, size_t up, size_t down, int n, bool before, bool more, const SsimRange &rg,
                                          double (*t)[kSsimCols])
{
    load_row(pl + i0 - up, n, before, more, rg, t[0]);
    load_row(pl + i0, n, before, more, rg, t[1]);
    load_row(pl + i0 + down, n, before, more, rg, t[2]);
}

// the window sums of the group's four pixels from the three rows of a product a * b (a == b: of squares; b == nullptr: of a itself)
__device__ __forceinline__ void window4(const double (*a)[kSsimCols], const double (*b)[kSsimCols], double *g)
{
#pragma clang fp contract(off)
    double col[kSsimCols];
#pragma unroll
    for (int i = 0; i < kSsimCols; ++i)
        col[i] = b ? ssim_tap3(a[0][i] * b[0][i], a[1][i] * b[1][i], a[2][i] * b[2][i]) : ssim_tap3(a[0][i], a[1][i], a[2][i]);
#pragma unroll
    for (int k = 0; k < kLossPx; ++k) g[k] = ssim_tap3(col[k], col[k + 1], col[k + 2]);
}

}  // namespace b2f
