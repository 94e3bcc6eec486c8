// Motion compensation as an output stage: the two neighbour frames of every triplet warped onto the reference frame by the flow
// (nn.BilinearSamplerBHWD with CUDA semantics behind the warpingUnit of models/pwc.lua:67-73) and the photometric error of those
// warps (criterions/OBCCriterion.lua:79-100 with criterions/penalty/L1_function.lua:20-21), on the device.  flow_warp_kernel reads flow,
// probabilities and the reference frame once, gathers the 2 x 3 x 4 taps of every pixel from the neighbours, writes the warped planes
// and reduces the per-pixel contributions of b2f_flowwarp.h, which the host entry (b2f_flow_warp_host) shares, into one record of
// B2F_PHOTO_WORDS integers per image: counters in registers, a wave reduction, the waves of a block through LDS, then at most one
// 64-bit atomicAdd per non-zero counter per block.  The sums are integers, so the record does not depend on the grid or on the order
// of the atomics.
#include "b2f_ctx.h"
#include "b2f_flowwarp.h"

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace b2f {

namespace {

constexpr int kPx = 4;        // consecutive pixels of a row per thread: one 16-byte load per float plane, one 4-byte load per byte plane
constexpr int kThreads = 256;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kWords = B2F_PHOTO_WORDS;

__device__ __forceinline__ float frame_value(float v) { return v; }
__device__ __forceinline__ float frame_value(unsigned char k) { return __fdiv_rn((float)k, 255.0f); }

// n (1..4) samples of a row at p as floats: one 16-byte (floats) or 4-byte (bytes) load where the address allows -- rows of odd W
// are not aligned --, scalar loads otherwise; v[n..] is left alone
__device__ __forceinline__ void load_px(const float *p, int n, float *v)
{
    if (n == kPx && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) v[k] = p[k];
}

__device__ __forceinline__ void load_px(const unsigned char *p, int n, float *v)
{
    if (n == kPx && ((uintptr_t)p & 3) == 0) {
        const uchar4 q = *reinterpret_cast<const uchar4 *>(p);
        v[0] = frame_value(q.x); v[1] = frame_value(q.y); v[2] = frame_value(q.z); v[3] = frame_value(q.w);
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) v[k] = frame_value(p[k]);
}

// the same for the stores of a warped plane: floats as they are, bytes quantised (warp_quantise)
__device__ __forceinline__ void store_px(float *p, int n, const float *v)
{
    if (n == kPx && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) p[k] = v[k];
}

__device__ __forceinline__ void store_px(unsigned char *p, int n, const float *v)
{
    if (n == kPx && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uchar4 *>(p) = make_uchar4(warp_quantise(v[0]), warp_quantise(v[1]), warp_quantise(v[2]), warp_quantise(v[3]));
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) p[k] = warp_quantise(v[k]);
}

// the counters of one direction in a thread: fewer than 2^28 pixels (the launcher's bound), so 32-bit counts and 64 bits for the sums
struct DirCounters {
    unsigned inside = 0, outside = 0, nonfinite = 0;
    unsigned long long charb = 0, sq = 0, ocharb = 0, weight = 0;
};

// One direction of a group: n pixels (x0 .., y) of the W x H image.  frm: the neighbour's three planes; fx, fy: the flow; ref: the
// reference values [channel][pixel]; pw: the direction's occlusion weights, read with has_w (a pointer that may be null would keep the
// array out of registers); out: the direction's three warped planes at the group's first pixel, or nullptr.
template <typename Tin, typename Tout, bool WantPhoto>
__device__ __forceinline__ void warp_direction(const Tin *frm, size_t hw, int W, int H, int x0, int y, int n, float k, const float *fx,
                                               const float *fy, const float (*ref)[kPx], const float *pw, bool has_w, Tout *out,
                                               DirCounters &cnt)
{
    WarpTaps t[kPx];
    float wv[3][kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        // a pixel past the row's end: zero flow at the group's first pixel, which is in the image; it is neither stored nor counted
        const bool live = j < n;
        t[j] = warp_taps(live ? fx[j] : 0.0f, live ? fy[j] : 0.0f, k, live ? x0 + j : x0, y, W, H);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            // the taps: every index lies in the image (warp_taps clamps; a NaN coordinate has xl = yt = 0 and loads nothing)
            const Tin *tl = frm + (size_t)c * hw + (size_t)t[j].yt * W + t[j].xl;
            const bool go = !t[j].nan;
            const float a = go ? frame_value(tl[0]) : 0.0f;
            const float b = (go && t[j].x1) ? frame_value(tl[1]) : 0.0f;
            const float cc = (go && t[j].y1) ? frame_value(tl[W]) : 0.0f;
            const float d = (go && t[j].x1 && t[j].y1) ? frame_value(tl[(size_t)W + 1]) : 0.0f;
            wv[c][j] = go ? warp_blend(t[j], a, b, cc, d) : 0.0f;
        }
        if (out) store_px(out + (size_t)c * hw, n, wv[c]);
    }
    if (WantPhoto) {
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            const float w3[3] = {wv[0][j], wv[1][j], wv[2][j]}, r3[3] = {ref[0][j], ref[1][j], ref[2][j]};
            const PixelPhoto s = photo_pixel(t[j], w3, r3, has_w, pw[j]);
            const bool live = j < n;
            cnt.inside += live ? s.inside : 0u;
            cnt.outside += live ? s.outside : 0u;
            cnt.nonfinite += live ? s.nonfinite : 0u;
            cnt.charb += live ? s.charb : 0ull;
            cnt.sq += live ? s.sq : 0ull;
            cnt.ocharb += live ? s.ocharb : 0ull;
            cnt.weight += live ? s.weight : 0ull;
        }
    }
}

// Image blockIdx.y: its blocks stride over the groups of kPx pixels of its rows.  im1 / im2 / im3: the frames of image 0, image b
// `stride` samples further; prob: the occlusion probabilities or nullptr; warped: n x 2 x 3 x hw or nullptr; photo[image] was zeroed
// on the stream (WantPhoto).  OwnPast: direction 0 (the past frame) takes its coordinate from past_flow, the model's own past flow
// (skip_ubfs of a Soft model, pwc.lua:425-432), instead of from flow; everything else of the direction is as without it.
template <typename Tin, typename Tout, bool WantPhoto, bool OwnPast>
__global__ void __launch_bounds__(kThreads) flow_warp_kernel(const float *flow, const float *past_flow, const float *prob, int H, int W,
                                                             float scale, const Tin *im1, const Tin *im2, const Tin *im3, size_t stride,
                                                             Tout *warped, unsigned long long *photo)
{
    const size_t b = blockIdx.y, hw = (size_t)H * W;
    const float *fxp = flow + b * 2 * hw, *fyp = fxp + hw;
    const float *bxp = OwnPast ? past_flow + b * 2 * hw : fxp, *byp = bxp + hw;
    const float *p0 = (WantPhoto && prob) ? prob + b * 2 * hw : nullptr, *p1 = p0 ? p0 + hw : nullptr;
    const Tin *past = im1 + b * stride, *refp = im2 + b * stride, *fut = im3 + b * stride;
    Tout *wout = warped ? warped + b * 6 * hw : nullptr;
    const size_t gpr = ((size_t)W + kPx - 1) / kPx, groups = gpr * (size_t)H;   // groups per row, per image
    DirCounters c0, c1;
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = W - x0 < kPx ? W - x0 : kPx;
        const size_t i0 = (size_t)y * W + x0;
        float fx[kPx] = {0.f, 0.f, 0.f, 0.f}, fy[kPx] = {0.f, 0.f, 0.f, 0.f}, q0[kPx] = {0.f, 0.f, 0.f, 0.f}, q1[kPx] = {0.f, 0.f, 0.f, 0.f};
        float ref[3][kPx] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        load_px(fxp + i0, n, fx);
        load_px(fyp + i0, n, fy);
        float bx[kPx] = {0.f, 0.f, 0.f, 0.f}, by[kPx] = {0.f, 0.f, 0.f, 0.f};
        if (OwnPast) {
            load_px(bxp + i0, n, bx);
            load_px(byp + i0, n, by);
        }
        if (WantPhoto) {
            if (p0) {
                load_px(p0 + i0, n, q0);
                load_px(p1 + i0, n, q1);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) load_px(refp + (size_t)c * hw + i0, n, ref[c]);
        }
        warp_direction<Tin, Tout, WantPhoto>(past, hw, W, H, x0, y, n, -scale, OwnPast ? bx : fx, OwnPast ? by : fy, ref, q1, p0 != nullptr, wout ? wout + i0 : nullptr, c0);
        warp_direction<Tin, Tout, WantPhoto>(fut, hw, W, H, x0, y, n, scale, fx, fy, ref, q0, p0 != nullptr,
                                             wout ? wout + 3 * hw + i0 : nullptr, c1);
    }
    if (!WantPhoto) return;
    // the record of this thread, then of its wave
    unsigned long long rec[kWords];
    rec[B2F_PHOTO_INSIDE] = c0.inside;         rec[B2F_PHOTO_INSIDE + 1] = c1.inside;
    rec[B2F_PHOTO_OUTSIDE] = c0.outside;       rec[B2F_PHOTO_OUTSIDE + 1] = c1.outside;
    rec[B2F_PHOTO_CHARB_Q30] = c0.charb;       rec[B2F_PHOTO_CHARB_Q30 + 1] = c1.charb;
    rec[B2F_PHOTO_SQ_Q30] = c0.sq;             rec[B2F_PHOTO_SQ_Q30 + 1] = c1.sq;
    rec[B2F_PHOTO_OCHARB_Q30] = c0.ocharb;     rec[B2F_PHOTO_OCHARB_Q30 + 1] = c1.ocharb;
    rec[B2F_PHOTO_WEIGHT_Q30] = c0.weight;     rec[B2F_PHOTO_WEIGHT_Q30 + 1] = c1.weight;
    rec[B2F_PHOTO_NONFINITE] = c0.nonfinite;   rec[B2F_PHOTO_NONFINITE + 1] = c1.nonfinite;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < kWords; ++j) rec[j] += __shfl_down(rec[j], off, kWave);
    }
    __shared__ unsigned long long part[kWaves][kWords];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kWords; ++j) part[wave][j] = rec[j];
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        unsigned long long sum = 0;
        for (int w = 0; w < kWaves; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(photo + b * kWords + threadIdx.x, sum);
    }
}

template <typename Tin, typename Tout, bool WantPhoto, bool OwnPast>
hipError_t launch_t(const float *flow, const float *past_flow, const float *prob, int n, int H, int W, float scale, const void *im1, const void *im2, const void *im3,
                    size_t stride, void *warped, unsigned long long *photo, unsigned bx, hipStream_t s)
{
    const size_t hw = (size_t)H * W;
    for (int b0 = 0; b0 < n; b0 += 65535) {   // grid.y holds 65535 images
        const int nb = std::min(n - b0, 65535);
        const size_t o = (size_t)b0;
        hipLaunchKernelGGL((flow_warp_kernel<Tin, Tout, WantPhoto, OwnPast>), dim3(bx, (unsigned)nb), dim3(kThreads), 0, s, flow + o * 2 * hw,
                           OwnPast ? past_flow + o * 2 * hw : nullptr,
                           prob ? prob + o * 2 * hw : nullptr, H, W, scale, (const Tin *)im1 + o * stride, (const Tin *)im2 + o * stride,
                           (const Tin *)im3 + o * stride, stride, warped ? (Tout *)warped + o * 6 * hw : nullptr,
                           photo ? photo + o * kWords : nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename Tin, typename Tout>
hipError_t launch_p(bool want_photo, const float *flow, const float *past_flow, const float *prob, int n, int H, int W, float scale,
                    const void *im1, const void *im2, const void *im3, size_t stride, void *warped, unsigned long long *photo, unsigned bx,
                    hipStream_t s)
{
    if (past_flow)
        return want_photo ? launch_t<Tin, Tout, true, true>(flow, past_flow, prob, n, H, W, scale, im1, im2, im3, stride, warped, photo, bx, s)
                          : launch_t<Tin, Tout, false, true>(flow, past_flow, prob, n, H, W, scale, im1, im2, im3, stride, warped, photo, bx, s);
    return want_photo ? launch_t<Tin, Tout, true, false>(flow, nullptr, prob, n, H, W, scale, im1, im2, im3, stride, warped, photo, bx, s)
                      : launch_t<Tin, Tout, false, false>(flow, nullptr, prob, n, H, W, scale, im1, im2, im3, stride, warped, photo, bx, s);
}

}  // namespace

hipError_t launch_flow_warp(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, const void *im1, const void *im2,
                            const void *im3, size_t image_stride, int in_kind, void *warped, int warped_kind, unsigned long long *photo,
                            hipStream_t s, const float *past_flow)
{
    const size_t hw = (size_t)H * W;
    const bool bin = in_kind == B2F_IN_U8, bout = warped_kind == B2F_IN_U8;
    if (n <= 0 || H <= 0 || W <= 0 || hw >= (size_t)kPhotoMaxPixels || !flow || !im1 || !im2 || !im3 || (!warped && !photo) ||
        image_stride < 3 * hw || (!bin && in_kind != B2F_IN_UNIT) || (!bout && warped_kind != B2F_IN_UNIT))
        return hipErrorInvalidValue;
    if (photo) {
        const hipError_t e = hipMemsetAsync(photo, 0, (size_t)n * kWords * sizeof(unsigned long long), s);
        if (e != hipSuccess) return e;
    }
    const size_t groups = (((size_t)W + kPx - 1) / kPx) * (size_t)H, blocks = (groups + kThreads - 1) / kThreads;
    // with the record a capped grid: about eight blocks per CU over the whole call, at most 1024 per image (a full-HD image alone
    // wraps the loop), so that few blocks add to a record; the warp alone takes a block per 256 groups
    const size_t cap = photo ? std::min<size_t>(1024, std::max<size_t>(8, 2048 / (size_t)n)) : (size_t)0x7fffffff;
    const unsigned bx = (unsigned)std::min(blocks, cap);
    const float scale = (float)flow_scale;
    const bool wp = photo != nullptr;
    if (bin)
        return bout ? launch_p<unsigned char, unsigned char>(wp, flow, past_flow, occ_prob, n, H, W, scale, im1, im2, im3, image_stride, warped, photo, bx, s)
                    : launch_p<unsigned char, float>(wp, flow, past_flow, occ_prob, n, H, W, scale, im1, im2, im3, image_stride, warped, photo, bx, s);
    return bout ? launch_p<float, unsigned char>(wp, flow, past_flow, occ_prob, n, H, W, scale, im1, im2, im3, image_stride, warped, photo, bx, s)
                : launch_p<float, float>(wp, flow, past_flow, occ_prob, n, H, W, scale, im1, im2, im3, image_stride, warped, photo, bx, s);
}

}  // namespace b2f

namespace {

// what every b2f_*flow_warp* entry checks before anything else
int check_flow_warp(const std::string &w, const void *flow, int n, int H, int W, double flow_scale, int in_kind, const void *im1, const void *im2,
                    const void *im3, const void *warped, const void *photo)
{
    if (n <= 0 || H <= 0 || W <= 0) return fail(w + ": bad shape");
    if ((long long)H * W >= kPhotoMaxPixels) return fail(w + ": images of 2^28 pixels or more are refused (the Q30 sums could overflow)");
    if (!(flow_scale > 0.0) || !std::isfinite(flow_scale)) return fail(w + ": flow_scale must be finite and > 0");
    if (in_kind != B2F_IN_UNIT && in_kind != B2F_IN_U8) return fail(w + ": in_kind must be B2F_IN_UNIT or B2F_IN_U8");
    if (!flow || !im1 || !im2 || !im3) return fail(w + ": null argument");
    if (!warped && !photo) return fail(w + ": at least one of warped and photo is required");
    return 0;
}

int warp_device(const char *who, b2f_ctx *c, const float *dev_flow, const float *dev_past_flow, const float *dev_occ_prob, int n, int H, int W,
                double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3, void *dev_warped,
                unsigned long long *dev_photo, void *stream);
int warp_op(const char *who, b2f_ctx *c, const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W, double flow_scale,
            int in_kind, const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo);

}  // namespace

extern "C" {

int b2f_flow_warp_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, int in_kind, const void *im1,
                       const void *im2, const void *im3, void *warped, unsigned long long *photo) try
{
    CHK(check_flow_warp(__func__, flow, n, H, W, flow_scale, in_kind, im1, im2, im3, warped, photo));
    flow_warp_host(flow, occ_prob, n, H, W, flow_scale, in_kind == B2F_IN_U8, im1, im2, im3, warped, photo);
    return 0;
}
B2F_CATCH("b2f_flow_warp_host")

int b2f_flow_warp_past_host(const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W, double flow_scale, int in_kind,
                            const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo) try
{
    CHK(check_flow_warp(__func__, flow, n, H, W, flow_scale, in_kind, im1, im2, im3, warped, photo));
    if (!past_flow) return fail(std::string(__func__) + ": null past_flow");
    flow_warp_host(flow, occ_prob, n, H, W, flow_scale, in_kind == B2F_IN_U8, im1, im2, im3, warped, photo, past_flow);
    return 0;
}
B2F_CATCH("b2f_flow_warp_past_host")

int b2f_flow_warp_device(b2f_ctx *c, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W, double flow_scale, int in_kind,
                         const void *dev_im1, const void *dev_im2, const void *dev_im3, void *dev_warped, unsigned long long *dev_photo,
                         void *stream) try
{
    return warp_device(__func__, c, dev_flow, nullptr, dev_occ_prob, n, H, W, flow_scale, in_kind, dev_im1, dev_im2, dev_im3, dev_warped,
                       dev_photo, stream);
}
B2F_CATCH("b2f_flow_warp_device")

int b2f_flow_warp_past_device(b2f_ctx *c, const float *dev_flow, const float *dev_past_flow, const float *dev_occ_prob, int n, int H, int W,
                              double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3, void *dev_warped,
                              unsigned long long *dev_photo, void *stream) try
{
    if (!dev_past_flow) return fail(std::string(__func__) + ": null past_flow");
    return warp_device(__func__, c, dev_flow, dev_past_flow, dev_occ_prob, n, H, W, flow_scale, in_kind, dev_im1, dev_im2, dev_im3, dev_warped,
                       dev_photo, stream);
}
B2F_CATCH("b2f_flow_warp_past_device")

int b2f_op_flow_warp(b2f_ctx *c, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, int in_kind, const void *im1,
                     const void *im2, const void *im3, void *warped, unsigned long long *photo) try
{
    return warp_op(__func__, c, flow, nullptr, occ_prob, n, H, W, flow_scale, in_kind, im1, im2, im3, warped, photo);
}
B2F_CATCH("b2f_op_flow_warp")

int b2f_op_flow_warp_past(b2f_ctx *c, const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                          int in_kind, const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo) try
{
    if (!past_flow) return fail(std::string(__func__) + ": null past_flow");
    return warp_op(__func__, c, flow, past_flow, occ_prob, n, H, W, flow_scale, in_kind, im1, im2, im3, warped, photo);
}
B2F_CATCH("b2f_op_flow_warp_past")

}  // extern "C"

namespace {

// b2f_flow_warp_device / b2f_flow_warp_past_device (dev_past_flow: nullptr without the own past flow)
int warp_device(const char *who, b2f_ctx *c, const float *dev_flow, const float *dev_past_flow, const float *dev_occ_prob, int n, int H, int W,
                double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3, void *dev_warped,
                unsigned long long *dev_photo, void *stream)
{
    const std::string w(who);
    CHK(check_flow_warp(w, dev_flow, n, H, W, flow_scale, in_kind, dev_im1, dev_im2, dev_im3, dev_warped, dev_photo));
    CHK(check_device_pointers(w, c, "b2f_op_flow_warp / b2f_flow_warp_host",
                              {dev_flow, dev_past_flow, dev_occ_prob, dev_im1, dev_im2, dev_im3, dev_warped, dev_photo}));
    HIPCHK(launch_flow_warp(dev_flow, dev_occ_prob, n, H, W, flow_scale, dev_im1, dev_im2, dev_im3, (size_t)3 * H * W, in_kind, dev_warped,
                            in_kind, dev_photo, stream ? (hipStream_t)stream : c->stream, dev_past_flow));
    return 0;
}

// b2f_op_flow_warp / b2f_op_flow_warp_past
int warp_op(const char *who, b2f_ctx *c, const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W, double flow_scale,
            int in_kind, const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo)
{
    CHK(check_flow_warp(who, flow, n, H, W, flow_scale, in_kind, im1, im2, im3, warped, photo));
    OpStage st(c, who);
    CHK(st.begin(true, "null context"));
    const size_t hw = (size_t)H * W, esz = in_kind == B2F_IN_U8 ? 1 : 4;
    const size_t nf = (size_t)n * 2 * hw, ni = (size_t)n * 3 * hw * esz, nw = 2 * ni, np = (size_t)n * B2F_PHOTO_WORDS;
    float *df, *db = nullptr, *dp = nullptr;
    unsigned char *d1, *d2, *d3, *dw = nullptr;   // bytes or floats, by in_kind
    unsigned long long *ds = nullptr;
    CHK(st.in(flow, nf, "flow", &df));
    if (past_flow) CHK(st.in(past_flow, nf, "past_flow", &db));
    if (occ_prob) CHK(st.in(occ_prob, nf, "occ_prob", &dp));
    CHK(st.in((const unsigned char *)im1, ni, "im1", &d1)); CHK(st.in((const unsigned char *)im2, ni, "im2", &d2));
    CHK(st.in((const unsigned char *)im3, ni, "im3", &d3));
    if (warped) CHK(st.out(nw, "warped", &dw));
    if (photo) CHK(st.out(np, "photo", &ds));
    HIPCHK(launch_flow_warp(df, dp, n, H, W, flow_scale, d1, d2, d3, 3 * hw, in_kind, dw, in_kind, ds, c->stream, db));
    CHK(st.finish());
    if (warped) CHK(st.get((unsigned char *)warped, dw, nw));
    return photo ? st.get(photo, ds, np) : 0;
}

}  // namespace
