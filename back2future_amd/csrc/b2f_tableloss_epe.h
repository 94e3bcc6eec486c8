// The supervised objective (-optimize epe, opts.lua:56) per pixel of one level of the output table: the masked end-point error of
// criterions/L2Criterion.lua:27-71 between the future flow and the sub-sampled ground truth (train.lua:296-314), and the same
// criterion between the occlusions and the two-channel target that train.lua:316-332 intends (t0 = [g == 0] + 0.5 [g == 0.5],
// t1 = [g == 1] + 0.5 [g == 0.5]; the Lua as written cannot run: it slices the labels to one channel and indexes channel 2 of it).
// One definition for the kernel (b2f_tableloss_epe.hip) and the host entry (b2f_host.cpp), in the manner of b2f_tableloss.h: fp64
// with contraction off, only + - * / and sqrt, which round correctly on both sides, and integer Q20 contributions, so that records and
// gradient are the same bits on the host and on the device.
#pragma once
#include "b2f_flowscore.h"

namespace b2f {

constexpr double kEpeEps = 1e-12;   // L2Criterion.lua:20

// what one pixel adds to the flow words (VALID, EPE_Q20, FLOW_NONFINITE) or to the occlusion words (LABELLED, OCC_Q20, OCC_NONFINITE)
// of its record (include/b2f.h, B2F_LOSS_EPE_*), and its two gradient elements before the rounding to fp32
struct EpeTerm {
    unsigned counted, nonfinite;
    unsigned long long q20;
    double g0, g1;
};

// L2Criterion on one pixel that its mask keeps: d = input - target (lines 36-38); the gradient (k * d_c) / (e + 1e-12) of lines 58-64
// with the factor k of train.lua:314 (times 1 / npixels with sizeAverage, lines 66-68).  k == 0 switches the gradient off: +0.0, not
// evaluated.  A non-finite e counts in nonfinite alone; its gradient expression is stored like any other.
B2F_HD inline EpeTerm epe_term(double d0, double d1, double k)
{
#pragma clang fp contract(off)
    EpeTerm r = {0u, 0u, 0ull, 0.0, 0.0};
    const double e = sqrt(d0 * d0 + d1 * d1);
    if (e - e == 0.0) {   // finite
        r.counted = 1u;
        r.q20 = (unsigned long long)((e < kScoreSaturate ? e : kScoreSaturate) * kScoreQ20 + 0.5);
    } else {
        r.nonfinite = 1u;
    }
    if (k != 0.0) {
        const double den = e + kEpeEps;
        r.g0 = (k * d0) / den;
        r.g1 = (k * d1) / den;
    }
    return r;
}

// the flow term of a valid pixel: f the future flow of level j, gt the true flow in pixels at the level's source pixel; div = 2^j with
// rescale_flow (train.lua:300-302), else 1
B2F_HD inline EpeTerm epe_flow_pixel(float f0, float f1, float gt0, float gt1, double flow_scale, double div, double k)
{
#pragma clang fp contract(off)
    const double g0 = ((double)gt0 / flow_scale) / div, g1 = ((double)gt1 / flow_scale) / div;
    return epe_term((double)f0 - g0, (double)f1 - g1, k);
}

// bytes 0 / 1 / 2 are the labels 0 / 0.5 / 1 (train.lua:324-325); anything else is unlabelled
B2F_HD inline bool epe_labelled(unsigned char label) { return label < 3; }

// the occlusion term of a labelled pixel
B2F_HD inline EpeTerm epe_occ_pixel(float o0, float o1, unsigned char label, double k)
{
#pragma clang fp contract(off)
    const double t0 = label == 0 ? 1.0 : (label == 1 ? 0.5 : 0.0), t1 = label == 2 ? 1.0 : (label == 1 ? 0.5 : 0.0);
    return epe_term((double)o0 - t0, (double)o1 - t1, k);
}

// k_j and k'_j of level j: base = epe * lw_j resp. occ * lw_j (lw_j = 1 with size_average, train.lua:60-64); with size_average divided by
// the number of valid resp. labelled source pixels of the level, 0 where there is none
B2F_HD inline double epe_factor(double base, bool size_average, double count)
{
#pragma clang fp contract(off)
    if (!size_average) return base;
    return count > 0.0 ? base / count : 0.0;
}

}  // namespace b2f
