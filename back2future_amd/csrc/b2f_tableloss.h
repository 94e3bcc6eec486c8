// The unsupervised validation loss of test.lua:266-297 (the -optimize pme branch) per pixel of one level of the output table: the
// contrast-sensitive smoothness of the flows and of the occlusions (criterions/SmoothnessCriterion.lua:45-63 with the L1 penalty of
// criterions/penalty/L1_function.lua:20 for flows and the quadratic one for occlusions, model.lua:216), the constant-velocity term
// (criterions/ConstVelCriterion.lua:36-38) and the occlusion prior (criterions/OcclusionPriorCriterion.lua:39).  The photometric term
// is photo_pixel of b2f_flowwarp.h on the table's own warped images.  One definition for the kernel (b2f_tableloss.hip) and the host
// entry (b2f_host.cpp): fp64 with fused multiply-add contraction off, an exponential written out from + - *, nearbyint and ldexp, and
// integer contributions (Q30 fixed point), so that a record is the same words on the host and on the device.
#pragma once
#include "b2f_flowwarp.h"

namespace b2f {

constexpr int kLossMaxLevels = 7;   // the level weights of test.lua:29-31

// E(t) = exp(t) for t <= 0 (test.lua:266-297 through SmoothnessCriterion.lua:58-59): t > 0 counts as 0, t < -708 gives 0, a NaN stays
// NaN.  k = nearbyint(t * log2 e), r = (t - k * ln2_hi) - k * ln2_lo, a degree-13 Taylor polynomial in Horner form, ldexp(p, k).
B2F_HD inline double loss_exp(double t)
{
#pragma clang fp contract(off)
    if (t != t) return t;
    if (t > 0.0) t = 0.0;
    if (t < -708.0) return 0.0;
    constexpr double c1 = 1.0, c2 = c1 / 2.0, c3 = c2 / 3.0, c4 = c3 / 4.0, c5 = c4 / 5.0, c6 = c5 / 6.0, c7 = c6 / 7.0, c8 = c7 / 8.0,
                     c9 = c8 / 9.0, c10 = c9 / 10.0, c11 = c10 / 11.0, c12 = c11 / 12.0, c13 = c12 / 13.0;
    const double k = nearbyint(t * 1.44269504088896338700e+00);
    const double r = (t - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = c13;
    p = p * r + c12;
    p = p * r + c11;
    p = p * r + c10;
    p = p * r + c9;
    p = p * r + c8;
    p = p * r + c7;
    p = p * r + c6;
    p = p * r + c5;
    p = p * r + c4;
    p = p * r + c3;
    p = p * r + c2;
    p = p * r + c1;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}

// forward differences of a pixel's three reference values to its contrast weight (SmoothnessCriterion.lua:58-59, cs = 20)
B2F_HD inline double loss_weight(double d0, double d1, double d2)
{
#pragma clang fp contract(off)
    return loss_exp(-20.0 * ((fabs(d0) + fabs(d1)) + fabs(d2)) / 3.0);
}

B2F_HD inline double loss_p1(double v)
{
#pragma clang fp contract(off)
    return sqrt(v * v + 1e-6);
}

// what one pixel adds to the record of its image and level besides the photo words (include/b2f.h, B2F_LOSS_*)
struct PixelLoss {
    unsigned long long smooth_flow, smooth_past, const_vel, smooth_occ, prior_occ;
    unsigned nonfinite;
};

// v: the pixel's values [f0 f1 p0 p1 o0 o1 R0 R1 R2], vx: the right neighbour's, vy: the lower neighbour's; has_x / has_y: that
// neighbour exists (a missing one gives a zero difference); past: the table has a past flow (p is not read otherwise)
B2F_HD inline PixelLoss loss_pixel(const float *v, const float *vx, const float *vy, bool has_x, bool has_y, bool past)
{
#pragma clang fp contract(off)
    double dx[9], dy[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        dx[c] = has_x ? (double)vx[c] - (double)v[c] : 0.0;
        dy[c] = has_y ? (double)vy[c] - (double)v[c] : 0.0;
    }
    const double wx = loss_weight(dx[6], dx[7], dx[8]), wy = loss_weight(dy[6], dy[7], dy[8]);
    const double s_flow = (loss_p1(dx[0]) * wx + loss_p1(dy[0]) * wy) + (loss_p1(dx[1]) * wx + loss_p1(dy[1]) * wy);
    const double s_occ = ((dx[4] * dx[4]) * wx + (dy[4] * dy[4]) * wy) + ((dx[5] * dx[5]) * wx + (dy[5] * dy[5]) * wy);
    const double prior = 1.0 - (double)v[4] * (double)v[5];
    PixelLoss r = {0ull, 0ull, 0ull, 0ull, 0ull, 0u};
    bool bad = s_flow != s_flow || s_occ != s_occ || prior != prior;
    if (s_flow == s_flow) r.smooth_flow = photo_q30(s_flow);
    if (s_occ == s_occ) r.smooth_occ = photo_q30(s_occ);
    if (prior == prior) r.prior_occ = photo_q30(prior);
    if (past) {
        const double s_past = (loss_p1(dx[2]) * wx + loss_p1(dy[2]) * wy) + (loss_p1(dx[3]) * wx + loss_p1(dy[3]) * wy);
        const double d0 = (double)v[0] - (double)v[2], d1 = (double)v[1] - (double)v[3];
        const double cv = sqrt(d0 * d0 + d1 * d1);
        bad = bad || s_past != s_past || cv != cv;
        if (s_past == s_past) r.smooth_past = photo_q30(s_past);
        if (cv == cv) r.const_vel = photo_q30(cv);
    }
    r.nonfinite = bad ? 1u : 0u;
    return r;
}

}  // namespace b2f
