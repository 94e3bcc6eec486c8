// Flow pictures as an output stage: flowX.xy2rgb (flowExtensions.lua:17-150) on the device.  flow_norm_max_kernel reduces the
// per-image maximum of the norm (the automatic maximum only), flow_rgb_kernel maps a planar n x 2 x H x W fp32 flow to bytes with the
// per-pixel function of b2f_flowcolor.h, which the host entry (b2f_flow_rgb_host) shares.  The arithmetic is fp64: in fp32 one byte
// in ~1e5 leaves the reference's value, in fp64 none does.
#include "b2f_ctx.h"
#include "b2f_flowcolor.h"

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace b2f {

namespace {

constexpr int kPx = 4;   // consecutive pixels of a row per thread: one 16-byte load per flow plane

// 4 floats at p: one 16-byte load where the address allows, n (1..4) scalar loads otherwise (the rest repeats the last one)
__device__ __forceinline__ void load_px(const float *p, int n, float *v)
{
    if (n == kPx && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kPx; ++k) v[k] = p[k < n ? k : n - 1];
}

// The largest norm of image blockIdx.y into mx[blockIdx.y], which the stream zeroed before: non-negative doubles order like their
// bit patterns, so the slot is a 64-bit unsigned maximum.  Every block contributes at least 1e-2, so the slot ends as the maximum
// xy2rgb divides by.  The norms are the correctly rounded values numpy computes, and a maximum does not depend on the order.
__global__ void __launch_bounds__(256) flow_norm_max_kernel(const float *flow, size_t hw, double *mx)
{
    const float *fx = flow + (size_t)blockIdx.y * 2 * hw, *fy = fx + hw;
    const size_t groups = (hw + kPx - 1) / kPx;
    double m = 1e-2;
    for (size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = gi * kPx;
        const int n = (int)(hw - i0 < (size_t)kPx ? hw - i0 : (size_t)kPx);
        float x[kPx], y[kPx];
        load_px(fx + i0, n, x);
        load_px(fy + i0, n, y);
        for (int k = 0; k < kPx; ++k) {
            const double v = flow_norm((double)x[k], (double)y[k]);
            m = v > m ? v : m;   // a NaN never enters
        }
    }
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off);
        m = o > m ? o : m;
    }
    __shared__ double wave_max[256 / 32];
    const int lane = threadIdx.x % warpSize, wave = threadIdx.x / warpSize, nwave = (blockDim.x + warpSize - 1) / warpSize;
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < nwave; ++k) m = wave_max[k] > m ? wave_max[k] : m;
        atomicMax(reinterpret_cast<unsigned long long *>(mx + blockIdx.y), (unsigned long long)__double_as_longlong(m));
    }
}

// A thread colours kPx consecutive pixels of one row of one image.  max_norm > 0: m = max(max_norm, 1e-2) with tanh; else
// m = mx[image] as flow_norm_max_kernel left it.  kPacked: n x H x W x 3 bytes, else n x 3 x H x W.
template <bool kPacked>
__global__ void __launch_bounds__(256) flow_rgb_kernel(const float *flow, int n_img, int H, int W, double max_norm, unsigned char *rgb,
                                                       double *mx)
{
    const size_t hw = (size_t)H * W;
    const size_t nq = ((size_t)W + kPx - 1) / kPx;   // pixel groups per row
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_img * H * nq) return;
    const size_t row = t / nq, b = row / H;
    const int j = (int)(row - b * H), i0 = (int)(t - row * nq) * kPx;
    const int n = min(kPx, W - i0);
    const bool saturate = max_norm > 0.0;
    const double m = saturate ? (max_norm > 1e-2 ? max_norm : 1e-2) : mx[b];
    if (saturate && mx && j == 0 && i0 == 0) mx[b] = m;   // the reference returns rgb, max
    const size_t d = (size_t)j * W + i0;               // first pixel of the group in a plane
    float x[kPx], y[kPx];
    load_px(flow + b * 2 * hw + d, n, x);
    load_px(flow + (b * 2 + 1) * hw + d, n, y);
    unsigned char c[3][kPx];
    for (int k = 0; k < kPx; ++k) {
        const Rgb8 v = flow_color((double)x[k], (double)y[k], m, saturate);
        c[0][k] = v.r; c[1][k] = v.g; c[2][k] = v.b;
    }
    if (kPacked) {
        unsigned char *o = rgb + (b * hw + d) * 3;
        if (n == kPx && ((uintptr_t)o & 3) == 0) {
            unsigned char e[3 * kPx];
            for (int k = 0; k < kPx; ++k)
                for (int ch = 0; ch < 3; ++ch) e[3 * k + ch] = c[ch][k];
            for (int q = 0; q < 3; ++q)
                reinterpret_cast<uchar4 *>(o)[q] = make_uchar4(e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]);
        } else {
            for (int k = 0; k < n; ++k)
                for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = c[ch][k];
        }
    } else {
        for (int ch = 0; ch < 3; ++ch) {
            unsigned char *o = rgb + (b * 3 + ch) * hw + d;
            if (n == kPx && ((uintptr_t)o & 3) == 0) {
                *reinterpret_cast<uchar4 *>(o) = make_uchar4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
            } else {
                for (int k = 0; k < n; ++k) o[k] = c[ch][k];
            }
        }
    }
}

}  // namespace

hipError_t launch_flow_rgb(const float *flow, int n, int H, int W, double max_norm, int layout, unsigned char *rgb, double *max_used,
                           hipStream_t s)
{
    const size_t hw = (size_t)H * W;
    if (!(max_norm > 0.0)) {
        if (!max_used) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(max_used, 0, (size_t)n * sizeof(double), s);
        if (e != hipSuccess) return e;
        const size_t groups = (hw + kPx - 1) / kPx;
        const unsigned bx = (unsigned)std::min<size_t>((groups + 255) / 256, 512);
        hipLaunchKernelGGL(flow_norm_max_kernel, dim3(bx, (unsigned)n), dim3(256), 0, s, flow, hw, max_used);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const size_t threads = (size_t)n * H * (((size_t)W + kPx - 1) / kPx);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (layout == B2F_RGB_PACKED)
        hipLaunchKernelGGL(flow_rgb_kernel<true>, grid, dim3(256), 0, s, flow, n, H, W, max_norm, rgb, max_used);
    else
        hipLaunchKernelGGL(flow_rgb_kernel<false>, grid, dim3(256), 0, s, flow, n, H, W, max_norm, rgb, max_used);
    return hipGetLastError();
}

}  // namespace b2f

namespace {

// what every b2f_*flow_rgb* entry checks before anything else
int check_flow_rgb(const std::string &w, const void *flow, int n, int H, int W, int layout, const void *rgb)
{
    if (layout != B2F_RGB_PLANAR && layout != B2F_RGB_PACKED) return fail(w + ": bad layout (B2F_RGB_PLANAR or B2F_RGB_PACKED)");
    if (n <= 0 || H <= 0 || W <= 0) return fail(w + ": bad shape");
    if (!flow || !rgb) return fail(w + ": null argument");
    return 0;
}

}  // namespace

extern "C" {

int b2f_flow_rgb_host(const float *flow, int n, int H, int W, double max_norm, int layout, unsigned char *rgb, double *max_used) try
{
    CHK(check_flow_rgb(__func__, flow, n, H, W, layout, rgb));
    flow_rgb_host(flow, n, H, W, max_norm, layout == B2F_RGB_PACKED, rgb, max_used);
    return 0;
}
B2F_CATCH("b2f_flow_rgb_host")

int b2f_flow_rgb_device(b2f_ctx *c, const float *dev_flow, int n, int H, int W, double max_norm, int layout, unsigned char *dev_rgb,
                        double *dev_max_used, void *stream) try
{
    const std::string w(__func__);
    CHK(check_flow_rgb(w, dev_flow, n, H, W, layout, dev_rgb));
    if (((uintptr_t)dev_flow | (uintptr_t)dev_rgb | (uintptr_t)dev_max_used) & 15) return fail(w + ": device buffers must be 16-byte aligned");
    if (!c) return fail(w + ": null context");
    HIPCHK(hipSetDevice(c->device));
    if (!dev_max_used && !(max_norm > 0.0)) {   // the automatic maxima need a place on the device
        DevWork &vm = c->vis_max;
        if ((size_t)n * sizeof(double) > vm.bytes) {
            if (vm.dev) {
                HIPCHK(hipDeviceSynchronize());   // an earlier call may still read it, on any stream
                HIPCHK(hipFree(vm.dev));
                vm.dev = nullptr; vm.bytes = 0;
            }
            HIPCHK(hipMalloc(&vm.dev, (size_t)n * sizeof(double)));
            vm.bytes = (size_t)n * sizeof(double);
        }
        dev_max_used = (double *)vm.dev;
    }
    HIPCHK(launch_flow_rgb(dev_flow, n, H, W, max_norm, layout, dev_rgb, dev_max_used, stream ? (hipStream_t)stream : c->stream));
    return 0;
}
B2F_CATCH("b2f_flow_rgb_device")

int b2f_op_flow_rgb(b2f_ctx *c, const float *flow, int n, int H, int W, double max_norm, int layout, unsigned char *rgb,
                    double *max_used) try
{
    CHK(check_flow_rgb(__func__, flow, n, H, W, layout, rgb));
    OpStage st(c, __func__);
    CHK(st.begin(true, "null context"));
    const size_t hw = (size_t)H * W, nf = (size_t)n * 2 * hw, nc = (size_t)n * 3 * hw;
    float *df;
    unsigned char *dc;
    double *dm;
    CHK(st.in(flow, nf, "flow", &df)); CHK(st.out(nc, "rgb", &dc)); CHK(st.out((size_t)n, "max_used", &dm));
    HIPCHK(launch_flow_rgb(df, n, H, W, max_norm, layout, dc, dm, c->stream));
    CHK(st.finish());
    CHK(st.get(rgb, dc, nc));
    return max_used ? st.get(max_used, dm, (size_t)n) : 0;
}
B2F_CATCH("b2f_op_flow_rgb")

}  // extern "C"
