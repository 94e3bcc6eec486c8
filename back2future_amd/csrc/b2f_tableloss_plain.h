// The photometric terms that do not mask occlusions (opts.lua:62: -pme_criterion BCC | SSIM | SSIML1; model.lua:149-159;
// criterions/MBCCriterion.lua:35-186, criterions/MSSIML1Criterion.lua:45-261) per pixel of one level of the output table: words 16 .. 29
// of the records of B2F_LOSS_PLAIN_WORDS words and the image planes of the gradient table (include/b2f.h).  One definition for the
// kernels (b2f_tableloss_plain.hip, b2f_tableloss_grad_plain.hip) and the host entries (b2f_host.cpp), in the manner of
// b2f_tableloss_ssim.h / b2f_tableloss_grad_ssim.h: fp64 with contraction off, photo_pixel, ssim_parts, loss_p1, grad_d1 and photo_q30
// as they are, integer Q30 contributions, a gradient element rounded to fp32 once, on store.
//
// Kept from the Lua:
//   - the inside test, the target coordinate and the level scale are OBCCriterion's (MBCCriterion.lua:70-87,
//     MSSIML1Criterion.lua:120-138): photo_pixel / warp_taps of b2f_flowwarp.h; a pixel-direction whose target leaves the image adds
//     nothing to the value and has a gradient of +0 (no penalty_out);
//   - the range of MSSIML1Criterion.lua:63-68 runs `for i = 2,#input`: beside R_j and the warped images it covers the occlusion tensor
//     and, on Soft tables, the past flow (the planes the range pass is given, not this file's concern);
//   - the gradient's centre tap gw = gc^2 everywhere and the missing 1 / (mx - mn) (b2f_tableloss_grad_ssim.h, 1 - 3).
#pragma once
#include "b2f_tableloss_grad_ssim.h"

namespace b2f {

// what one pixel of one direction adds to words 16 .. 19 of its record, and whether it counts
struct PixelPlainRaw {
    unsigned long long l1, sq;
    bool counted;
};

// ph: photo_pixel of the direction with the occlusion weight of words 6 .. 9: its `inside` is PHOTO_INSIDE, its charb / sq are q(B1) /
// q(B2) on the raw planes (MBCCriterion.lua:65-66 with the L1 resp. the criterion's own quadratic penalty), without the weight
B2F_HD inline PixelPlainRaw plain_raw(const PixelPhoto &ph)
{
    PixelPlainRaw o = {0ull, 0ull, ph.inside != 0u};
    if (o.counted) {
        o.l1 = ph.charb;
        o.sq = ph.sq;
    }
    return o;
}

// what it adds to words 20 .. 25
struct PixelPlainSsim {
    unsigned long long ssim, l1n;
    unsigned nonfinite;
};

// S = (s_0 + s_1) + s_2 with s_c = ssim_term of channel c, B = (e_0 + e_1) + e_2 with e_c = loss_p1(x_c - y_c) on the normalised planes
// (MSSIML1Criterion.lua:117, no occlusion weight); counted: plain_raw's; ok: the range is usable (S and B are not read otherwise)
B2F_HD inline PixelPlainSsim plain_ssim(bool counted, double S, double B, bool ok)
{
#pragma clang fp contract(off)
    PixelPlainSsim o = {0ull, 0ull, 0u};
    if (!counted) return o;
    if (!ok || S != S || B != B) {
        o.nonfinite = 1u;
        return o;
    }
    o.ssim = photo_q30(S);
    o.l1n = photo_q30(B);
    return o;
}

// what the options add to the coefficients of a level: the SSIM + L1 coefficients (alpha, beta, which are evaluated) and, in pl, the
// criterion and the penalty; grad_plain_occ_on says whether the occlusion planes have a term (else they are +0.0 everywhere)
enum { kGradPlainSsim = 1, kGradPlainQuad = 2 };
struct GradPlainCoef {
    GradSsimCoef s;
    unsigned pl;
};

B2F_HD inline bool grad_plain_occ_on(const GradCoef &k) { return (k.on & (kGradSmoothOcc | kGradPrior)) != 0; }

// G_iw_d[c] of BCC from the raw values (MBCCriterion.lua:146-149,175,179-181): der = D1 or 2 delta
B2F_HD inline float grad_plain_bcc(const GradPlainCoef &k, bool inside, float warped, float ref)
{
#pragma clang fp contract(off)
    if (!inside) return 0.0f;
    const double d = (double)warped - (double)ref;
    return (float)(k.s.k.k_p * ((k.pl & kGradPlainQuad) ? 2.0 * d : grad_d1(d)));
}

// G_iw_d[c] of SSIM / SSIML1 from T_c = grad_ssim_channel(..).t (MSSIML1Criterion.lua:224,250,254-257)
B2F_HD inline float grad_plain_ssim(const GradPlainCoef &k, bool inside, double t)
{
#pragma clang fp contract(off)
    return inside ? (float)(k.s.k.k_p * t) : 0.0f;
}

// G_o[c]: the photometric criterion's part is exactly zero (gradInput[1]:fill(0)); what remains is grad_occ without its first term
B2F_HD inline float grad_plain_occ(const GradCoef &k, double S, float other)
{
#pragma clang fp contract(off)
    GradSum r;
    if (k.on & kGradSmoothOcc) r.add(k.k_so * S);
    if (k.on & kGradPrior) r.add(k.k_pr * (1.0 - (double)other));
    return (float)r.g;
}

}  // namespace b2f
