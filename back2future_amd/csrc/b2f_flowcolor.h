// The colour of one flow vector: flowX.xy2rgb (flowExtensions.lua:17-150) per pixel, as flow_io.xy2rgb restates it
// (computeNorm, computeAngle, field2rgb, hsl2rgb), quantised to bytes the way flow_io.save_image / image.save do.  One function
// for the kernel (b2f_vis.hip) and the host entry (b2f_host.cpp).  Everything is fp64 in the operation order of flow_io.py with
// fused multiply-add contraction off, so that sqrt, /, *, + and - round exactly as numpy's do: the pictures are then the
// yardstick's bytes up to the last bit of atan / tanh, and the automatic maximum is numpy's double.
#pragma once
#include <cmath>

#if defined(__HIPCC__) && defined(__HIP__)
#define B2F_HD __host__ __device__
#else
#define B2F_HD
#endif

namespace b2f {

struct Rgb8 {
    unsigned char r, g, b;
};

// computeNorm: sqrt(y * y + x * x), this order
B2F_HD inline double flow_norm(double x, double y)
{
#pragma clang fp contract(off)
    return sqrt(y * y + x * x);
}

// image.save: floor(clip(v, 0, 1) * 255 + 0.5); NaN becomes 0
B2F_HD inline unsigned char flow_quantise(double v)
{
#pragma clang fp contract(off)
    v = v > 0.0 ? (v < 1.0 ? v : 1.0) : 0.0;
    return (unsigned char)(int)(v * 255.0 + 0.5);
}

// x, y: the flow widened to double; m: the maximum the norm is divided by (already >= 1e-2); saturate: tanh the saturation
// (a caller-given maximum) or not (the automatic one, where norm <= m)
B2F_HD inline Rgb8 flow_color(double x, double y, double m, bool saturate)
{
#pragma clang fp contract(off)
    // computeAngle: degrees in 0..360; the x == 0 cases come first (zero flow: 90)
    double angle;
    if (x == 0.0) {
        angle = y >= 0.0 ? 90.0 : 270.0;
    } else {
        const double h = atan(fabs(y / x)) * (180.0 / 3.14159265358979323846);
        angle = x >= 0.0 ? (y >= 0.0 ? h : 360.0 - h) : (y >= 0.0 ? 180.0 - h : 180.0 + h);
    }
    // field2rgb: hue = angle / 360, saturation = norm / max, lightness = 1 - saturation / 2
    double s = flow_norm(x, y) / m;
    if (saturate) s = tanh(s);
    const double hue = angle / 360.0, l = 1.0 - 0.5 * s;
    // image.hsl2rgb
    if (s == 0.0) {
        const unsigned char grey = flow_quantise(l);
        return {grey, grey, grey};
    }
    const double q = l < 0.5 ? l * (1.0 + s) : l + s - l * s, p = 2.0 * l - q;
    const double ts[3] = {hue + 1.0 / 3.0, hue, hue - 1.0 / 3.0};
    unsigned char c[3];
    for (int k = 0; k < 3; ++k) {
        double t = ts[k];
        if (t < 0.0) t = t + 1.0;
        if (t > 1.0) t = t - 1.0;
        double v;
        if (t < 1.0 / 6.0) v = p + (q - p) * 6.0 * t;
        else if (t < 1.0 / 2.0) v = q;
        else if (t < 2.0 / 3.0) v = p + (q - p) * (2.0 / 3.0 - t) * 6.0;
        else v = p;
        c[k] = flow_quantise(v);
    }
    return {c[0], c[1], c[2]};
}

}  // namespace b2f
