// The gradient of the -optimize pme objective with respect to the output table: what train.lua:428-468 adds into `gradOutputs` on one
// level, per element.  The specification is the reference's updateGradInput functions, not the derivative of their outputs:
// criterions/SmoothnessCriterion.lua:85-102 (L1 penalty for the flows, quadratic for the occlusions), ConstVelCriterion.lua:59-65,
// OBCCriterion.lua:147-237 (L1 penalty) and OcclusionPriorCriterion.lua:64-65.  Three places where the two differ, all kept:
//   1. the prior returns 1 - o[other]; the derivative of 1 - o0 * o1 is -o[other] (larger by the constant k_pr on both channels, which
//      the softmax below the occlusions cancels);
//   2. a pixel-direction whose target leaves the image adds penalty_out = 1 to the occlusion gradient of channel 1 - d, where the
//      forward value has a constant;
//   3. with size_average the constant-velocity gradient is divided by h w, its output by 2 h w.
// One definition for the kernel (b2f_tableloss_grad.hip) and the host entry (b2f_host.cpp), on the pieces of b2f_tableloss.h and
// b2f_flowwarp.h: fp64 with contraction off, loss_exp / loss_weight / loss_p1 as they are, the fp32 coordinate of warp_taps.  An
// element is summed in fp64 and rounded to fp32 once, on store, so host and kernel give the same bits (the reference accumulates in
// fp32 and rounds after every add).
#pragma once
#include "b2f_tableloss.h"

namespace b2f {

// the terms of one level: coefficient = (level weight * option weight) * norm, formed in fp64 on the host (table_loss_grad_coef);
// a term whose option weight is exactly 0 has its bit clear in `on`, is not evaluated and adds nothing (train.lua:458,465)
enum { kGradSmooth = 1, kGradConstVel = 2, kGradPhoto = 4, kGradSmoothOcc = 8, kGradPrior = 16 };
struct GradCoef {
    double k_s, k_cv, k_p, k_so, k_pr;
    unsigned on;
};

// the enabled terms of an element, added left to right; an element without one is +0.0
struct GradSum {
    double g = 0.0;
    bool any = false;
    B2F_HD inline void add(double t)
    {
#pragma clang fp contract(off)
        g = any ? g + t : t;
        any = true;
    }
};

B2F_HD inline double grad_d1(double v)   // the derivative of P1 (L1_function.lua:25)
{
#pragma clang fp contract(off)
    return v / sqrt(v * v + 1e-6);
}

// a(x, y) (lo = F(x, y), hi = F(x + 1, y), wgt = wx(x, y)) or b(x, y) over rows: D(hi - lo) * wgt where the pair exists, else
// exactly 0 without a multiplication (SmoothnessCriterion.lua:85-86: the penalty's derivative of a zero difference is 0)
template <bool Quad>
B2F_HD inline double grad_edge(bool has, float lo, float hi, double wgt)
{
#pragma clang fp contract(off)
    if (!has) return 0.0;
    const double v = (double)hi - (double)lo;
    return (Quad ? 2.0 * v : grad_d1(v)) * wgt;
}

// the contrast weight of the pair (lo, hi) of reference pixels (b2f_tableloss.h: loss_weight); 1 where there is no pair (not read)
B2F_HD inline double grad_weight(bool has, float lo0, float hi0, float lo1, float hi1, float lo2, float hi2)
{
#pragma clang fp contract(off)
    if (!has) return 1.0;
    return loss_weight((double)hi0 - (double)lo0, (double)hi1 - (double)lo1, (double)hi2 - (double)lo2);
}

// S(F)(x, y) from a(x, y), a(x - 1, y), b(x, y), b(x, y - 1) (SmoothnessCriterion.lua:100-102)
B2F_HD inline double grad_s(double a, double al, double b, double bu)
{
#pragma clang fp contract(off)
    return (((-a) + al) - b) + bu;
}

// CV_c of a pixel (ConstVelCriterion.lua:59-65)
B2F_HD inline void grad_const_vel(float f0, float f1, float p0, float p1, double *cv)
{
#pragma clang fp contract(off)
    const double d0 = (double)f0 - (double)p0, d1 = (double)f1 - (double)p1;
    const double den = sqrt(d0 * d0 + d1 * d1) + 1e-12;
    cv[0] = d0 / den;
    cv[1] = d1 / den;
}

// G_f[c] (sign = +1) or G_p[c] (sign = -1) from S of the plane and CV_c; cv_on: the table has a past flow
B2F_HD inline float grad_flow(const GradCoef &k, double S, double cv, bool cv_on, bool minus)
{
#pragma clang fp contract(off)
    GradSum r;
    if (k.on & kGradSmooth) r.add(k.k_s * S);
    if (cv_on && (k.on & kGradConstVel)) {
        const double t = k.k_cv * cv;
        r.add(minus ? -t : t);
    }
    return (float)r.g;
}

// direction d of a pixel (OBCCriterion.lua:147-237): inside = m_d, warped / ref its three values of iw_d and R_j, ow = o[1 - d].
// po: PO_{1-d}; giw[c]: G_iw_d[c], rounded
B2F_HD inline void grad_photo(const GradCoef &k, bool inside, const float *warped, const float *ref, float ow, double *po, float *giw)
{
#pragma clang fp contract(off)
    if (!inside) {
        *po = 1.0;
        giw[0] = giw[1] = giw[2] = 0.0f;
        return;
    }
    const double d0 = (double)warped[0] - (double)ref[0], d1 = (double)warped[1] - (double)ref[1], d2 = (double)warped[2] - (double)ref[2];
    const double s0 = loss_p1(d0), s1 = loss_p1(d1), s2 = loss_p1(d2), o = (double)ow;
    *po = (s0 + s1) + s2;
    giw[0] = (float)(k.k_p * ((d0 / s0) * o));
    giw[1] = (float)(k.k_p * ((d1 / s1) * o));
    giw[2] = (float)(k.k_p * ((d2 / s2) * o));
}

// G_o[c] from PO_c, S(o, c) with the quadratic penalty and the other channel's value
B2F_HD inline float grad_occ(const GradCoef &k, double po, double S, float other)
{
#pragma clang fp contract(off)
    GradSum r;
    if (k.on & kGradPhoto) r.add(k.k_p * po);
    if (k.on & kGradSmoothOcc) r.add(k.k_so * S);
    if (k.on & kGradPrior) r.add(k.k_pr * (1.0 - (double)other));
    return (float)r.g;
}

}  // namespace b2f
