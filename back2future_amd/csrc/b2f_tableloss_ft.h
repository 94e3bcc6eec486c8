// The terms the two Soft models were fine-tuned on (README.md:89-102: -smooth_second_order, -pme_criterion OBGCC) per pixel of one
// level of the output table, beside those of b2f_tableloss.h (test.lua:266-297): the contrast-sensitive second-order smoothness of
// criterions/SecondOrderSmoothnessCriterion.lua:45-65 and the gradient-constancy sums of criterions/OBGCCriterion.lua:67-68,91-105,
// both with the L1 penalty of criterions/penalty/L1_function.lua:20.  One definition for the kernel (b2f_tableloss_ft.hip) and the
// host entry (b2f_host.cpp), in the manner of b2f_tableloss.h: fp64 with contraction off, loss_exp, loss_p1 and photo_q30 as they
// are, integer Q30 contributions only.  photo_q30 saturates at 16, which was sized for the brightness term; a second difference of
// a flow or the three-channel sum of gradient differences of normalized images (up to about 28) can pass it, so each product of a
// penalty and its weight is rounded on its own here and a pixel adds the sum of those integers: no term of plausible inputs saturates.
#pragma once
#include "b2f_tableloss.h"

namespace b2f {

// what one pixel adds to words 16, 17 and 22 of its record (include/b2f.h, B2F_LOSS_FT_*)
struct PixelSmooth2 {
    unsigned long long flow, past;
    unsigned nonfinite;
};

// the channel mean of |a - b| over the three reference values (SecondOrderSmoothnessCriterion.lua:55-58, torch.mean over dim 2)
B2F_HD inline double ft_mean_abs(const float *a, const float *b)
{
#pragma clang fp contract(off)
    return ((fabs((double)a[0] - (double)b[0]) + fabs((double)a[1] - (double)b[1])) + fabs((double)a[2] - (double)b[2])) / 3.0;
}

// 2 f(x) - f(x-1) - f(x+1) in the order of SecondOrderSmoothnessCriterion.lua:45-46
B2F_HD inline double ft_second(float c, float a, float b)
{
#pragma clang fp contract(off)
    return (2.0 * (double)c - (double)a) - (double)b;
}

// v: the pixel's values [f0 f1 p0 p1 R0 R1 R2]; vl, vr, vu, vd: those of its left, right, upper and lower neighbour, read only where
// has_* says the neighbour exists; past: the table has a past flow (p is not read otherwise).  The second difference is 0 unless both
// neighbours of the axis exist (lines 45-46: a border pixel still adds P1(0) times its weight); the weight's exponent takes
// |R(x) - R(x-1)| wherever a left neighbour exists (lines 55-56) and |R(x) - R(x+1)| only on interior pixels (lines 57-58).  Maps
// the reference cannot slice (h < 3 or w < 3) follow the same rule: a missing neighbour gives no term.
B2F_HD inline PixelSmooth2 smooth2_pixel(const float *v, const float *vl, const float *vr, const float *vu, const float *vd, bool has_l, bool has_r,
                                         bool has_u, bool has_d, bool past)
{
#pragma clang fp contract(off)
    const bool in_x = has_l && has_r, in_y = has_u && has_d;
    const double igx = (has_l ? ft_mean_abs(v + 4, vl + 4) : 0.0) + (in_x ? ft_mean_abs(v + 4, vr + 4) : 0.0);
    const double igy = (has_u ? ft_mean_abs(v + 4, vu + 4) : 0.0) + (in_y ? ft_mean_abs(v + 4, vd + 4) : 0.0);
    const double wx = loss_exp(-20.0 * igx), wy = loss_exp(-20.0 * igy);
    double g[4][2];   // per channel f0 f1 p0 p1: gx, gy
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool read = past || c < 2;
        g[c][0] = (read && in_x) ? ft_second(v[c], vl[c], vr[c]) : 0.0;
        g[c][1] = (read && in_y) ? ft_second(v[c], vu[c], vd[c]) : 0.0;
    }
    PixelSmooth2 r = {0ull, 0ull, 0u};
    double t[4][2];   // the four products of a flow: channel, axis
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        t[c][0] = loss_p1(g[c][0]) * wx;
        t[c][1] = loss_p1(g[c][1]) * wy;
    }
    const double s_flow = (t[0][0] + t[0][1]) + (t[1][0] + t[1][1]);   // NaN exactly when one of its products is
    bool bad = s_flow != s_flow;
    if (!bad) r.flow = (photo_q30(t[0][0]) + photo_q30(t[0][1])) + (photo_q30(t[1][0]) + photo_q30(t[1][1]));
    if (past) {
        const double s_past = (t[2][0] + t[2][1]) + (t[3][0] + t[3][1]);
        if (s_past == s_past) r.past = (photo_q30(t[2][0]) + photo_q30(t[2][1])) + (photo_q30(t[3][0]) + photo_q30(t[3][1]));
        bad = bad || s_past != s_past;
    }
    r.nonfinite = bad ? 1u : 0u;
    return r;
}

// what one pixel of one direction adds to words 18 .. 21 and 23 of its record
struct PixelGrad {
    unsigned long long ogx, ogy;
    unsigned nonfinite;
};

// iw / r: the pixel's three warped and reference values, *x the right neighbour's, *y the lower neighbour's (read only where has_x /
// has_y; the forward differences of both images are 0 in the last column and row, OBGCCriterion.lua:67-68,91-92); counted: the
// pixel-direction is one of PHOTO_INSIDE (photo_pixel of b2f_flowwarp.h); p: the occlusion weight of the direction (lines 116,121)
B2F_HD inline PixelGrad grad_pixel(const float *iw, const float *iwx, const float *iwy, const float *r, const float *rx, const float *ry, bool has_x,
                                   bool has_y, bool counted, float p)
{
#pragma clang fp contract(off)
    PixelGrad o = {0ull, 0ull, 0u};
    if (!counted) return o;
    double ex[3], ey[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double dx = has_x ? ((double)iwx[c] - (double)iw[c]) - ((double)rx[c] - (double)r[c]) : 0.0;
        const double dy = has_y ? ((double)iwy[c] - (double)iw[c]) - ((double)ry[c] - (double)r[c]) : 0.0;
        ex[c] = loss_p1(dx);
        ey[c] = loss_p1(dy);
    }
    const double w = (double)p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ex[c] = w * ex[c];
        ey[c] = w * ey[c];
    }
    const double gx = (ex[0] + ex[1]) + ex[2], gy = (ey[0] + ey[1]) + ey[2];   // NaN exactly when one of its products is
    if (gx != gx || gy != gy) {
        o.nonfinite = 1u;
        return o;
    }
    o.ogx = (photo_q30(ex[0]) + photo_q30(ex[1])) + photo_q30(ex[2]);
    o.ogy = (photo_q30(ey[0]) + photo_q30(ey[1])) + photo_q30(ey[2]);
    return o;
}

}  // namespace b2f
