// The occlusion-aware SSIM + L1 photometric term (opts.lua:62: -pme_criterion OSSIM | OSSIML1; model.lua:172-179;
// criterions/OSSIML1Criterion.lua:47-163) per pixel of one level of the output table, beside the terms of b2f_tableloss.h: words 16 .. 25
// of the records of B2F_LOSS_SSIM_WORDS words (include/b2f.h).  One definition for the kernels (b2f_tableloss_ssim.hip) and the host
// entry (b2f_host.cpp), in the manner of b2f_tableloss_ft.h: fp64 with contraction off, loss_p1 and photo_q30 as they are, integer Q30
// contributions only.
//
// The window.  OSSIML1Criterion.lua:38-44 filters with image.gaussian{size = 3, normalize = true} behind SpatialReplicationPadding(1).
// The torch `image` package is not part of the reference tree, so its weights are restated here from that package's documented
// defaults and have not been compared with a Torch7 installation: sigma = 0.25 * size, centre on the middle tap, an unnormalised tap
// at distance d being exp(-(d / 0.75)^2 / 2), the nine taps normalised to sum 1.  That kernel is the outer product of the 1-D
// weights (ge, gc, ge) with e = exp(-8/9).  A pin against Torch7 corrects the one line that defines kSsimE.
#pragma once
#include "b2f_tableloss.h"

namespace b2f {

constexpr double kSsimE = 0.41111229050718745;   // exp(-8/9): the tap one pixel off the centre before normalisation
constexpr double kSsimGe = kSsimE / (1.0 + 2.0 * kSsimE), kSsimGc = 1.0 / (1.0 + 2.0 * kSsimE);   // the 1-D weights, edge and centre
constexpr double kSsimC1 = 1e-4, kSsimC2 = 9e-4;   // OSSIML1Criterion.lua:31-32

// The order-preserving unsigned encoding of a float: a < b as floats exactly when ssim_enc(a) < ssim_enc(b) as integers (-0 below +0).
// A minimum and a maximum taken on it are exact and do not depend on the order of the values.  No non-NaN value encodes to 0 or to
// 0xffffffff, which ssim_dec turns into NaNs: the range of no values.
B2F_HD inline unsigned ssim_enc(float v)
{
    unsigned u;
    __builtin_memcpy(&u, &v, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

B2F_HD inline unsigned ssim_dec_bits(unsigned e) { return (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e; }

B2F_HD inline float ssim_dec(unsigned e)
{
    const unsigned u = ssim_dec_bits(e);
    float v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// the range of one image and level as the pixels use it
struct SsimRange {
    double mn, span;
    bool ok;   // mx > mn and both finite: otherwise every counted pixel-direction is non-finite
};

B2F_HD inline SsimRange ssim_range(float mn, float mx)
{
#pragma clang fp contract(off)
    SsimRange r;
    r.mn = (double)mn;
    r.span = (double)mx - (double)mn;
    r.ok = mx > mn && mn - mn == 0.0f && mx - mx == 0.0f;
    return r;
}

// t = (v - mn) / (mx - mn) (OSSIML1Criterion.lua:62-67)
B2F_HD inline double ssim_norm(float v, const SsimRange &r)
{
#pragma clang fp contract(off)
    return ((double)v - r.mn) / r.span;
}

// three taps of the 1-D window in its fixed order: a column from the rows above, at and below, or the window from its three columns
B2F_HD inline double ssim_tap3(double a, double c, double b)
{
#pragma clang fp contract(off)
    return (kSsimGe * a + kSsimGc * c) + kSsimGe * b;
}

// l, cs and their denominators A, Bd of one channel from its five window sums: mu_x = G(x), mu_y = G(y), gxx = G(x x), gyy = G(y y),
// gxy = G(x y) (OSSIML1Criterion.lua:115-116; the gradient of b2f_tableloss_grad_ssim.h divides by A and Bd again)
struct SsimParts {
    double l, cs, A, Bd;
};

B2F_HD inline SsimParts ssim_parts(double mu_x, double mu_y, double gxx, double gyy, double gxy)
{
#pragma clang fp contract(off)
    const double xx = mu_x * mu_x, yy = mu_y * mu_y, xy = mu_x * mu_y;
    const double s_x = gxx - xx, s_y = gyy - yy, s_xy = gxy - xy;
    SsimParts p;
    p.A = (xx + yy) + kSsimC1;
    p.Bd = (s_x + s_y) + kSsimC2;
    p.l = (2.0 * xy + kSsimC1) / p.A;
    p.cs = (2.0 * s_xy + kSsimC2) / p.Bd;
    return p;
}

// 1 - l * cs of one channel
B2F_HD inline double ssim_term(double mu_x, double mu_y, double gxx, double gyy, double gxy)
{
#pragma clang fp contract(off)
    const SsimParts p = ssim_parts(mu_x, mu_y, gxx, gyy, gxy);
    return 1.0 - p.l * p.cs;
}

// what one pixel of one direction adds to words 16 .. 21 of its record
struct PixelSsim {
    unsigned long long ssim, l1n;
    unsigned nonfinite;
};

// S = (s_0 + s_1) + s_2 with s_c = ssim_term of channel c, B = (e_0 + e_1) + e_2 with e_c = loss_p1(x_c - y_c) on the pixel's normalised
// warped and reference values; counted: the pixel-direction is one of PHOTO_INSIDE (photo_pixel of b2f_flowwarp.h); ok: the range is
// usable (SsimRange::ok; S and B are not read otherwise); p: the occlusion weight of the direction (OSSIML1Criterion.lua:137,142)
B2F_HD inline PixelSsim ssim_pixel(double S, double B, bool counted, bool ok, float p)
{
#pragma clang fp contract(off)
    PixelSsim o = {0ull, 0ull, 0u};
    if (!counted) return o;
    if (!ok) {
        o.nonfinite = 1u;
        return o;
    }
    const double w = (double)p, ws = w * S, wb = w * B;
    if (ws != ws || wb != wb) {
        o.nonfinite = 1u;
        return o;
    }
    o.ssim = photo_q30(ws);
    o.l1n = photo_q30(wb);
    return o;
}

}  // namespace b2f
