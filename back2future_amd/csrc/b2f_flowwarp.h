// Motion compensation of one pixel: the warp of a neighbour frame by the flow -- nn.BilinearSamplerBHWD with CUDA semantics
// (extras/stnbhwd/BilinearSamplerBHWD.cu:6-20,88-104) behind the warpingUnit of models/pwc.lua:67-73 -- and what the pixel adds to
// the photometric record of its image (criterions/OBCCriterion.lua:79-100 with the penalty of criterions/penalty/L1_function.lua:20-21).  One
// definition for the kernel (b2f_warp.hip) and the host entry (b2f_host.cpp).  The warp is fp32 and the error fp64, both with fused
// multiply-add contraction off, so that every operation rounds the same on the host and on the device; what a pixel contributes is
// integers only (counts, and the errors in Q30 fixed point), so a sum of pixels does not depend on its order.
#pragma once
#include <cmath>

#if defined(__HIPCC__) && defined(__HIP__)
#define B2F_HD __host__ __device__
#else
#define B2F_HD
#endif

namespace b2f {

// where one pixel of one direction samples its neighbour frame
struct WarpTaps {
    bool nan;                    // the coordinate is NaN: the warped value is 0, nothing is loaded (xl = yt = 0, no second taps)
    bool inside;                 // 0 <= xc <= W - 1 and 0 <= yc <= H - 1 before the clamp (OBCCriterion.lua:97-100, 0-based)
    bool x1, y1;                 // the right / lower taps lie in the image (a tap outside contributes 0)
    int xl, yt;                  // the top-left tap, always in the image
    float wtl, wtr, wbl, wbr;    // the four weights
};

constexpr double kPhotoSaturate = 16.0;        // with it 2^28 pixels cannot overflow 64 bits of Q30
constexpr double kPhotoQ30 = 1073741824.0;
constexpr long long kPhotoMaxPixels = 1ll << 28;

// fx, fy: raw network flow at pixel (x, y) of a W x H image; k: -flow_scale for the past frame, +flow_scale for the future one
B2F_HD inline WarpTaps warp_taps(float fx, float fy, float k, int x, int y, int W, int H)
{
#pragma clang fp contract(off)
    const float u = fx * k, v = fy * k;
    float xc = u + (float)x, yc = v + (float)y;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    WarpTaps t;
    t.nan = xc != xc || yc != yc;
    t.inside = xc >= 0.0f && xc <= xmax && yc >= 0.0f && yc <= ymax;
    if (t.nan) {
        t.x1 = t.y1 = false;
        t.xl = t.yt = 0;
        t.wtl = t.wtr = t.wbl = t.wbr = 0.0f;
        return t;
    }
    if (xc < 0.0f) xc = 0.0f;
    if (xc > xmax) xc = xmax;
    if (yc < 0.0f) yc = 0.0f;
    if (yc > ymax) yc = ymax;
    const float xf = floorf(xc), yf = floorf(yc);
    const float xw = 1.0f - (xc - xf), yw = 1.0f - (yc - yf);
    // (the integer clamp only matters where W - 1 is no fp32 number: an index never leaves the image)
    t.xl = (int)xf < W - 1 ? (int)xf : W - 1;
    t.yt = (int)yf < H - 1 ? (int)yf : H - 1;
    t.x1 = t.xl + 1 <= W - 1;
    t.y1 = t.yt + 1 <= H - 1;
    t.wtl = xw * yw;
    t.wtr = (1.0f - xw) * yw;
    t.wbl = xw * (1.0f - yw);
    t.wbr = (1.0f - xw) * (1.0f - yw);
    return t;
}

// the four taps' values (0 for a tap outside the image) to the warped value, added left to right
B2F_HD inline float warp_blend(const WarpTaps &t, float tl, float tr, float bl, float br)
{
#pragma clang fp contract(off)
    return t.wtl * tl + t.wtr * tr + t.wbl * bl + t.wbr * br;
}

// a warped value as image.save writes it: round to nearest byte of the value clamped to [0, 1]; a NaN gives 0
B2F_HD inline unsigned char warp_quantise(float v)
{
#pragma clang fp contract(off)
    return v > 0.0f ? (v < 1.0f ? (unsigned char)floorf(v * 255.0f + 0.5f) : (unsigned char)255) : (unsigned char)0;
}

B2F_HD inline unsigned long long photo_q30(double t)
{
#pragma clang fp contract(off)
    return (unsigned long long)((t < 0.0 ? 0.0 : t < kPhotoSaturate ? t : kPhotoSaturate) * kPhotoQ30 + 0.5);
}

// what one pixel of one direction adds to the record of its image (include/b2f.h, B2F_PHOTO_*)
struct PixelPhoto {
    unsigned inside, outside, nonfinite;
    unsigned long long charb, sq, ocharb, weight;
};

// t: the pixel's taps; warped / ref: its three warped (float, before any quantisation) and reference values; has_w / p: the occlusion
// weight of the direction (p1 for the past frame, p0 for the future one; OBCCriterion.lua:86,91)
B2F_HD inline PixelPhoto photo_pixel(const WarpTaps &t, const float *warped, const float *ref, bool has_w, float p)
{
#pragma clang fp contract(off)
    PixelPhoto r = {0u, 0u, 0u, 0ull, 0ull, 0ull, 0ull};
    if (t.nan) {
        r.nonfinite = 1u;
        return r;
    }
    if (!t.inside) {
        r.outside = 1u;
        return r;
    }
    // (written out channel by channel: no indexed copy of the six values)
    const double d0 = (double)warped[0] - (double)ref[0], d1 = (double)warped[1] - (double)ref[1], d2 = (double)warped[2] - (double)ref[2];
    const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2;
    const double e = (sqrt(q0 + 1e-6) + sqrt(q1 + 1e-6)) + sqrt(q2 + 1e-6);
    const double sq = (q0 + q1) + q2;
    const double w = has_w ? (double)p : 0.0, we = w * e;
    if (e != e || we != we || w != w) {
        r.nonfinite = 1u;
        return r;
    }
    r.inside = 1u;
    r.charb = photo_q30(e);
    r.sq = photo_q30(sq);
    if (has_w) {
        r.ocharb = photo_q30(we);
        r.weight = photo_q30(w);
    }
    return r;
}

}  // namespace b2f
