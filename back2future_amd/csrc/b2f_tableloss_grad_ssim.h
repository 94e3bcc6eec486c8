// The gradient of the occlusion-aware SSIM + L1 photometric term (opts.lua:62: -pme_criterion OSSIM | OSSIML1) with respect to the
// output table: b2f_tableloss_grad.h / b2f_tableloss_grad_ft.h with the photometric term replaced.  The specification is the
// reference's updateGradInput, criterions/OSSIML1Criterion.lua:165-302, combined with the other terms as train.lua:428-468 combines
// them -- not the derivative of the records' value.  Five places where the two differ, all kept (include/b2f.h):
//   1. lines 217-218 differentiate the pixel's own window term with respect to the pixel's own value; the eight neighbouring windows
//      that also hold the pixel are dropped;
//   2. under replication padding a border pixel occurs several times in its own window (a corner pixel with the weight (gc + ge)^2);
//      line 216 takes the centre tap gw = gc * gc everywhere;
//   3. the gradient is with respect to the normalised image: the factor 1 / (mx - mn) and the dependence of mn and mx on the inputs
//      are absent, and the range is not checked for usability (a zero or non-finite span follows IEEE);
//   4. a pixel-direction whose target leaves the image adds penalty_out = 1 to the occlusion gradient (lines 244-245, 272-273);
//   5. the occlusion prior's 1 - o[other] comes along unchanged (b2f_tableloss_grad.h).
// One definition for the kernel (b2f_tableloss_grad_ssim.hip) and the host entry (b2f_host.cpp): fp64 with contraction off, the
// window sums, ssim_parts and loss_p1 of b2f_tableloss_ssim.h and grad_d1 as they are; an element is summed in fp64 and rounded to
// fp32 once, on store.
#pragma once
#include "b2f_tableloss_grad.h"
#include "b2f_tableloss_ssim.h"

namespace b2f {

constexpr double kSsimGw = kSsimGc * kSsimGc;   // the 2-D window's centre tap (OSSIML1Criterion.lua:204,216)

// what the SSIM + L1 options add to the coefficients of a level: alpha, beta = 1.0 - alpha, and which of the two terms are evaluated
// (a weight of exactly 0: not evaluated)
enum { kGradSsimAlpha = 1, kGradSsimBeta = 2 };
struct GradSsimCoef {
    GradCoef k;
    double alpha, beta;
    unsigned ss;
};

// Q_c = dl * cs + l * dcs of one channel (lines 217-218, 222) from its window sums' parts, the pixel's normalised warped (x) and
// reference (y) value and the two means
B2F_HD inline double grad_ssim_q(const SsimParts &p, double x, double y, double mu_x, double mu_y)
{
#pragma clang fp contract(off)
    const double dl = ((2.0 * kSsimGw) * (mu_y - mu_x * p.l)) / p.A;
    const double dcs = ((2.0 * kSsimGw) * ((y - mu_y) - p.cs * (x - mu_x))) / p.Bd;
    return dl * p.cs + p.l * dcs;
}

// what one channel of a pixel-direction gives: T_c (line 222), and its 1 - l * cs and P1(x - y) for the sums S and B of line 224; a
// term that is not enabled is not evaluated and left +0.0
struct GradSsimChannel {
    double t, s, e;
};

B2F_HD inline GradSsimChannel grad_ssim_channel(const GradSsimCoef &k, double x, double y, double mu_x, double mu_y, double gxx, double gyy, double gxy)
{
#pragma clang fp contract(off)
    GradSsimChannel r = {0.0, 0.0, 0.0};
    GradSum t;
    if (k.ss & kGradSsimAlpha) {
        const SsimParts p = ssim_parts(mu_x, mu_y, gxx, gyy, gxy);
        r.s = 1.0 - p.l * p.cs;
        t.add(-(k.alpha * grad_ssim_q(p, x, y, mu_x, mu_y)));
    }
    if (k.ss & kGradSsimBeta) {
        const double d = x - y;
        r.e = loss_p1(d);
        t.add(k.beta * grad_d1(d));
    }
    r.t = t.g;
    return r;
}

// G_iw_d[c] from T_c: inside = m_d, ow = o[1 - d] (lines 249, 257, 289)
B2F_HD inline float grad_ssim_image(const GradSsimCoef &k, bool inside, double t, float ow)
{
#pragma clang fp contract(off)
    return inside ? (float)(k.k.k_p * (t * (double)ow)) : 0.0f;
}

// PO_{1-d} from S = (s_0 + s_1) + s_2 and B = (e_0 + e_1) + e_2 (lines 224, 243-245)
B2F_HD inline double grad_ssim_po(const GradSsimCoef &k, bool inside, double S, double B)
{
#pragma clang fp contract(off)
    if (!inside) return 1.0;
    GradSum r;
    if (k.ss & kGradSsimAlpha) r.add(k.alpha * S);
    if (k.ss & kGradSsimBeta) r.add(k.beta * B);
    return r.g;
}

}  // namespace b2f
