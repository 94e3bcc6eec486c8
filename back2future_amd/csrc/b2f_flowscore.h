// The score of one pixel against ground truth: the masked end-point error of test.lua:183-261 (criterions/L2Criterion.lua:36-38,
// times flownet_factor), split by the ground-truth occlusion label, KITTI's outlier rule "Fl", and the occlusion confusion matrix
// of test.lua:236-259.  One definition for the kernel (b2f_score.hip) and the host entry (b2f_host.cpp).  The flow arithmetic is
// fp64 with fused multiply-add contraction off, so that *, -, + and sqrt round the same on the host and on the device; what a pixel
// contributes is integers only (counts, and the error in Q20 fixed point), so a sum of pixels does not depend on its order.
#pragma once
#include <cmath>

#if defined(__HIPCC__) && defined(__HIP__)
#define B2F_HD __host__ __device__
#else
#define B2F_HD
#endif

namespace b2f {

// what one pixel adds to the record of its image (include/b2f.h, B2F_SCORE_*)
struct PixelScore {
    int bucket;                 // 0 occluded "bwd", 1 visible, 2 occluded "fwd", 3 unlabelled: the words the next three go to
    unsigned counted;           // 1: a valid pixel with a finite error
    unsigned outlier;           // 1: err > 3 px and err > 5 % of the ground truth's magnitude
    unsigned nonfinite;         // 1: a valid pixel whose error is NaN; nothing else of it is counted
    unsigned long long q20;     // round(min(err, 65536) * 2^20)
};

constexpr double kScoreSaturate = 65536.0;   // px: with it 2^28 pixels cannot overflow 64 bits of Q20
constexpr double kScoreQ20 = 1048576.0;
constexpr long long kScoreMaxPixels = 1ll << 28;

// fx, fy: raw network flow; gx, gy: ground truth in pixels; valid: the pixel's mask byte (NULL mask: 1); label: its gt_occ byte
// (NULL plane: 3).  An invalid pixel's values enter nothing that is counted.
B2F_HD inline PixelScore score_flow_pixel(float fx, float fy, double flow_scale, float gx, float gy, unsigned char valid, unsigned char label)
{
#pragma clang fp contract(off)
    PixelScore r = {label < 3 ? (int)label : 3, 0u, 0u, 0u, 0ull};
    if (!valid) return r;
    const double dx = (double)fx * flow_scale - (double)gx, dy = (double)fy * flow_scale - (double)gy;
    const double err = sqrt(dy * dy + dx * dx);
    const double mag = sqrt((double)gy * (double)gy + (double)gx * (double)gx);
    if (err != err) {
        r.nonfinite = 1u;
        return r;
    }
    r.counted = 1u;
    r.q20 = (unsigned long long)((err < kScoreSaturate ? err : kScoreSaturate) * kScoreQ20 + 0.5);
    r.outlier = (err > 3.0 && err > 0.05 * mag) ? 1u : 0u;
    return r;
}

// test.lua:236: the class of an occlusion estimate, round((1 - p0) + p1) in fp32, halves away from zero, clamped to 0 .. 2 (the
// sum is a whole number after roundf, so two comparisons clamp it; a NaN is class 0)
B2F_HD inline int score_occ_class(float p0, float p1)
{
#pragma clang fp contract(off)
    const float c = roundf((1.0f - p0) + p1);
    return c >= 2.0f ? 2 : (c >= 1.0f ? 1 : 0);
}

}  // namespace b2f
