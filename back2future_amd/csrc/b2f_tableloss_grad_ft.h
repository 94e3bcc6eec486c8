// The gradient of the Soft models' fine-tuning objective (README.md:89-102: -smooth_second_order, -pme_criterion OBGCC) with respect to
// the output table: b2f_tableloss_grad.h with two terms replaced where their flag is set.  The specification is again the reference's
// updateGradInput functions: criterions/SecondOrderSmoothnessCriterion.lua:77-104 and criterions/OBGCCriterion.lua:151-300 (both with
// the L1 penalty), combined as train.lua:428-468 combines them.  Four places where OBGCC's differ from the derivative of its output,
// all kept (include/b2f.h): alpha multiplies the gradient although updateOutput never applies it; a neighbour's contribution to a
// pixel's image gradient is masked and weighted with the pixel's own m_d and o; the occlusion gradient combines the penalty values
// with the derivative's signs; gamma is honoured as given.  One definition for the kernel (b2f_tableloss_grad_ft.hip) and the host
// entry (b2f_host.cpp): fp64 with contraction off, the second difference and contrast mean of b2f_tableloss_ft.h, loss_exp, loss_p1
// and grad_d1 as they are; an element is summed in fp64 and rounded to fp32 once, on store.
#pragma once
#include "b2f_tableloss_ft.h"
#include "b2f_tableloss_grad.h"

namespace b2f {

// what the fine-tuning flags add to the coefficients of a level: which criterion serves the flows' smoothness and the photometric
// term, OBGCC's three weights and which of its terms are evaluated (a weight of exactly 0: not evaluated)
enum { kGradFtSecond = 1, kGradFtObgcc = 2, kGradFtAlpha = 4, kGradFtBeta = 8, kGradFtGamma = 16 };
struct GradFtCoef {
    GradCoef k;
    double alpha, beta, gamma;
    unsigned ft;
};

// the sum of |hi - lo| over the three reference values of a pair of pixels, one channel at a time: (|d0| + |d1|) + |d2|, three times
// the channel mean of SecondOrderSmoothnessCriterion.lua:55-58 and the sum under loss_weight's exponent (b2f_tableloss.h).  The
// difference of two floats is exact in fp64, so the order of the pair does not matter.
B2F_HD inline double grad_abs3_add(double acc, bool first, float lo, float hi)
{
#pragma clang fp contract(off)
    const double v = fabs((double)hi - (double)lo);
    return first ? v : acc + v;
}

// the first-order weight of a pair from its sum (loss_weight of b2f_tableloss.h)
B2F_HD inline double grad_weight_sum(double a)
{
#pragma clang fp contract(off)
    return loss_exp(-20.0 * a / 3.0);
}

// the second-order weight of an interior pixel from the sums of its pairs with the pixel before and after it on the axis
// (SecondOrderSmoothnessCriterion.lua:55-61; smooth2_pixel of b2f_tableloss_ft.h with both neighbours)
B2F_HD inline double grad2_weight_sums(double al, double ar)
{
#pragma clang fp contract(off)
    return loss_exp(-20.0 * (al / 3.0 + ar / 3.0));
}

// the same from the three reference values of the pixel before (l), the pixel (c) and the pixel after it (r)
B2F_HD inline double grad2_weight(float l0, float c0, float r0, float l1, float c1, float r1, float l2, float c2, float r2)
{
#pragma clang fp contract(off)
    const double al = grad_abs3_add(grad_abs3_add(grad_abs3_add(0.0, true, l0, c0), false, l1, c1), false, l2, c2);
    const double ar = grad_abs3_add(grad_abs3_add(grad_abs3_add(0.0, true, c0, r0), false, c1, r1), false, c2, r2);
    return grad2_weight_sums(al, ar);
}

// qx(x, y) (lo = F(x - 1, y), c = F(x, y), hi = F(x + 1, y), wgt = wx(x, y)) or qy over rows: D1 of the second difference times the
// weight on interior pixels; not formed elsewhere (lines 87-88 on the slices of lines 92-97)
B2F_HD inline double grad2_q(bool interior, float lo, float c, float hi, double wgt)
{
#pragma clang fp contract(off)
    if (!interior) return 0.0;
    return grad_d1(ft_second(c, lo, hi)) * wgt;
}

// S2(F)(x, y) in the order of lines 92-97; a q that is not formed is +0.0
B2F_HD inline double grad2_s(double qy, double qx, double qyd, double qxr, double qyu, double qxl)
{
#pragma clang fp contract(off)
    return (((((2.0 * qy) + (2.0 * qx)) - qyd) - qxr) - qyu) - qxl;
}

// OBCC channel by channel (grad_photo of b2f_tableloss_grad.h for a pixel inside): G_iw_d[c], and P1(delta_c) into the sum over the
// channels, channel 0 first
B2F_HD inline float obcc_image(const GradCoef &k, float warped, float ref, float ow, bool first, double *sum)
{
#pragma clang fp contract(off)
    const double d = (double)warped - (double)ref, s = loss_p1(d);
    *sum = first ? s : *sum + s;
    return (float)(k.k_p * ((d / s) * (double)ow));
}

// the forward difference of the error of channel c (OBGCCriterion.lua:183-184,194-195,205,210; dx_c / dy_c of b2f_tableloss_ft.h):
// i / r the pixel's warped and reference value, in / rn those of the next pixel on the axis; 0 where there is none
B2F_HD inline double obgcc_e(bool has, float i, float in, float r, float rn)
{
#pragma clang fp contract(off)
    return has ? ((double)in - (double)i) - ((double)rn - (double)r) : 0.0;
}

// one channel's five error values of a pixel-direction: delta, ey(x, y), ey(x, y - 1), ex(x, y), ex(x - 1, y); has_u / has_l: the
// shifted ones exist (they are not read otherwise)
struct ObgccErr {
    double d, ey, eyu, ex, exl;
};

// the enabled terms of lines 202-212 (F = D1) or 215-219 (F = the sum of P1 over the channels) from their five values, left to right
B2F_HD inline double obgcc_sum(const GradFtCoef &k, bool has_u, bool has_l, double d, double ey, double eyu, double ex, double exl)
{
#pragma clang fp contract(off)
    GradSum r;
    if (k.ft & kGradFtAlpha) r.add(k.alpha * d);
    if (k.ft & kGradFtGamma) {
        r.add(-(k.gamma * ey));
        if (has_u) r.add(k.gamma * eyu);
    }
    if (k.ft & kGradFtBeta) {
        r.add(-(k.beta * ex));
        if (has_l) r.add(k.beta * exl);
    }
    return r.g;
}

// G_iw_d[c] of a pixel inside (lines 202-212, 254, 287-289): e the channel's five values, ow = o[1 - d]
B2F_HD inline float obgcc_image(const GradFtCoef &k, bool has_u, bool has_l, const ObgccErr &e, float ow)
{
#pragma clang fp contract(off)
    const bool a = (k.ft & kGradFtAlpha) != 0, g = (k.ft & kGradFtGamma) != 0, b = (k.ft & kGradFtBeta) != 0;
    const double t = obgcc_sum(k, has_u, has_l, a ? grad_d1(e.d) : 0.0, g ? grad_d1(e.ey) : 0.0, (g && has_u) ? grad_d1(e.eyu) : 0.0,
                               b ? grad_d1(e.ex) : 0.0, (b && has_l) ? grad_d1(e.exl) : 0.0);
    return (float)(k.k.k_p * (t * (double)ow));
}

// the channel's P1 values into the five sums over the channels of lines 215-219, channel 0 first: (P1_0 + P1_1) + P1_2
B2F_HD inline void obgcc_p1_add(const GradFtCoef &k, bool has_u, bool has_l, const ObgccErr &e, bool first, double *s)
{
#pragma clang fp contract(off)
    const bool a = (k.ft & kGradFtAlpha) != 0, g = (k.ft & kGradFtGamma) != 0, b = (k.ft & kGradFtBeta) != 0;
    const double v[5] = {a ? loss_p1(e.d) : 0.0, g ? loss_p1(e.ey) : 0.0, (g && has_u) ? loss_p1(e.eyu) : 0.0, b ? loss_p1(e.ex) : 0.0,
                         (b && has_l) ? loss_p1(e.exl) : 0.0};
#pragma unroll
    for (int i = 0; i < 5; ++i) s[i] = first ? v[i] : s[i] + v[i];
}

// PO_{1-d} of a pixel inside from the five sums
B2F_HD inline double obgcc_po(const GradFtCoef &k, bool has_u, bool has_l, const double *s)
{
    return obgcc_sum(k, has_u, has_l, s[0], s[1], s[2], s[3], s[4]);
}

}  // namespace b2f
