// Device side of the computeFlow boundary (/root/reference/back2future.lua:48-93): what the reference does on the
// host around model:forward -- ColorNormalize, image.scale(..., W, H) 'bilinear' down to multiples of 64, and
// after the forward pass image.scale(..., 'simple') back to the input size and the 0.6666 thresholds, one output kernel for
// every entry point -- runs here on the uploaded planes, so the host only moves bytes (and, on the f64 entries, widens the
// flow, b2f_pipeline.hip).  The arithmetic
// is the CPU routines' (oracle/b2f_oracle.c) operation for operation: every output element is produced by one
// thread with the same sequence of IEEE fp32 operations (the file is built with -ffp-contract=off and correctly
// rounded division), so the results are bit-identical to the CPU ones.
#include "b2f_internal.h"

namespace b2f {

// element `di` of image.scale's separable line resampler [3P torch/image generic/image.c scaleLinear_rowcol]:
// up = align-corners lerp with the last sample copied, down = fractional box average, float accumulators.
// `fetch(i)` returns source sample i of the line.
template <class F>
__device__ __forceinline__ float scale_line_elem(F fetch, long slen, long dlen, long di)
{
    if (dlen > slen) {
        if (di == dlen - 1) return fetch(slen - 1);
        if (slen == 1) return fetch(0);
        const float scale = (float)(slen - 1) / (float)(dlen - 1);
        float f = di * scale;
        const long i0 = (long)f;
        f -= i0;
        return (1 - f) * fetch(i0) + f * fetch(i0 + 1);
    }
    if (dlen == slen) return fetch(di);
    const float scale = (float)slen / (float)dlen;
    // the running (a_i, a_f) of the sequential loop is the previous element's (e_i, e_f) = split(di * scale)
    float a_f = di * scale;
    const long a_i = (long)a_f;
    a_f -= a_i;
    float e_f = (di + 1) * scale;
    const long e_i = (long)e_f;
    e_f -= e_i;
    float acc = (1 - a_f) * fetch(a_i), wsum = 1 - a_f;
    for (long si = a_i + 1; si < e_i; ++si) { acc += fetch(si); wsum += 1; }
    if (e_i < slen) { acc += e_f * fetch(e_i); wsum += e_f; }
    return acc / wsum;
}

// rows: [planes][Hs][Ws] -> [planes][Hs][Wd]; normalize = ColorNormalize on the fly (plane % 3 = colour)
__global__ void scale_rows_kernel(const float *src, int normalize, long planes, int Hs, int Ws, int Wd, float *dst)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)planes * Hs * Wd) return;
    const long dx = (long)(i % Wd);
    const size_t row = i / Wd;                 // plane * Hs + y
    const int ch = (int)((row / Hs) % 3);
    const float *s = src + row * Ws;
    dst[i] = scale_line_elem([&](long k) { const float v = s[k]; return normalize ? color_normalize(v, ch) : v; }, Ws, Wd, dx);
}

// columns: [planes][Hs][Wd] -> [planes][Hd][Wd]
__global__ void scale_cols_kernel(const float *src, long planes, int Hs, int Hd, int Wd, float *dst)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)planes * Hd * Wd) return;
    const int x = (int)(i % Wd);
    const size_t t = i / Wd;
    const long dy = (long)(t % Hd);
    const size_t plane = t / Hd;
    const float *s = src + plane * Hs * Wd + x;
    dst[i] = scale_line_elem([&](long k) { return s[k * Wd]; }, Hs, Hd, dy);
}

hipError_t launch_image_scale(const float *src, int normalize, long planes, int Hs, int Ws, float *tmp, float *dst,
                              int Hd, int Wd, hipStream_t s)
{
    const size_t n1 = (size_t)planes * Hs * Wd, n2 = (size_t)planes * Hd * Wd;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, src, normalize, planes, Hs, Ws, Wd, tmp);
    hipLaunchKernelGGL(scale_cols_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, tmp, planes, Hs, Hd, Wd, dst);
    return hipGetLastError();
}

// back2future.lua:77-93 for every computeFlow entry: image.scale(..., 'simple') of the network's outputs from fh x fw to H0 x W0
// and the thresholds:
//   flow      (float)((double)est[1] * sc)   (sc_w for channel 0, sc_h for 1): the f64 value rounded to nearest.  The f64 entries
//             pass sc = 1 -- (float)((double)f * 1.0) == f -- and their host threads form the :double() copy times sc_w / sc_h
//             (:80-84): half the bytes on the link
//   occ_prob  skip_occs[3] (occ: [B][2][fh][fw]; est[3] of a Soft model, est[2] of a Hard one)
//   fwd_occ / bwd_occ  ge(est[3][2], 0.6666) / ge(est[3][1], 0.6666)
// Any output may be nullptr (the host path passes no flow when H0 x W0 is the network size: it downloads the network's planes).
// One thread per kOutPx consecutive pixels of an output row: 16-byte stores (4-byte for the
// masks) where the row holds them and the address is aligned, scalar stores for a row's tail and misaligned rows.  When
// the column map is the identity (fw == W0, so the 4 source samples are consecutive and 16-byte aligned) the planes are
// read with 16-byte loads too (kVec: a separate instantiation, so that the compiler cannot fold the two load paths into one).
constexpr int kOutPx = 4;

template <bool kVec>
__device__ __forceinline__ float4 gather4(const float *p, const size_t *s)
{
    if (kVec) return *reinterpret_cast<const float4 *>(p + s[0]);
    return make_float4(p[s[0]], p[s[1]], p[s[2]], p[s[3]]);
}

__device__ __forceinline__ void store4(float *dst, float4 v, int n)
{
    if (n == kOutPx && ((uintptr_t)dst & 15) == 0) {
        *reinterpret_cast<float4 *>(dst) = v;
        return;
    }
    const float e[4] = {v.x, v.y, v.z, v.w};
    for (int k = 0; k < n; ++k) dst[k] = e[k];
}

__device__ __forceinline__ void store4(unsigned char *dst, const unsigned char *e, int n)
{
    if (n == kOutPx && ((uintptr_t)dst & 3) == 0) {
        *reinterpret_cast<uchar4 *>(dst) = make_uchar4(e[0], e[1], e[2], e[3]);
        return;
    }
    for (int k = 0; k < n; ++k) dst[k] = e[k];
}

template <bool kVec>
__global__ void outputs_f32_kernel(const float *flow_net, const float *occ, const float *est3, int est3_ch, int B, int fh, int fw,
                                   int H0, int W0, double sc_w, double sc_h, float *flow, float *occ_prob, unsigned char *fwd_occ,
                                   unsigned char *bwd_occ)
{
    const size_t hw0 = (size_t)H0 * W0, hw = (size_t)fh * fw;
    const size_t nq = ((size_t)W0 + kOutPx - 1) / kOutPx;   // pixel groups per output row
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * H0 * nq) return;
    const size_t row = t / nq, b = row / H0;
    const int j = (int)(row - b * H0), i0 = (int)(t - row * nq) * kOutPx;
    const int n = min(kOutPx, W0 - i0);
    // image.scale 'simple' [3P]: src index = (long)(dst * (float)src_len / dst_len), clamped
    const float scx = (float)fw / (float)W0, scy = (float)fh / (float)H0;
    long jj = (long)((float)j * scy);
    if (jj > fh - 1) jj = fh - 1;
    size_t s[kOutPx];
    for (int k = 0; k < kOutPx; ++k) {
        const int i = i0 + min(k, n - 1);   // the tail repeats its last pixel: in-bounds loads, never stored
        long ii = (long)((float)i * scx);
        if (ii > fw - 1) ii = fw - 1;
        s[k] = (size_t)jj * fw + ii;
    }
    const size_t d = (size_t)j * W0 + i0;   // first pixel of the group in an output plane
    if (flow) {
        const float *fn = flow_net + b * 2 * hw;
        for (int ch = 0; ch < 2; ++ch) {
            const float4 v = gather4<kVec>(fn + ch * hw, s);
            const double sc = ch == 0 ? sc_w : sc_h;
            store4(flow + (b * 2 + ch) * hw0 + d,
                   make_float4((float)((double)v.x * sc), (float)((double)v.y * sc), (float)((double)v.z * sc), (float)((double)v.w * sc)), n);
        }
    }
    if (occ_prob) {
        const float *op = occ + b * 2 * hw;
        for (int ch = 0; ch < 2; ++ch) store4(occ_prob + (b * 2 + ch) * hw0 + d, gather4<kVec>(op + ch * hw, s), n);
    }
    if (fwd_occ || bwd_occ) {
        const float *e3 = est3 + b * est3_ch * hw;
        for (int ch = 0; ch < 2; ++ch) {   // bwd_occ = ge(est[3][1]), fwd_occ = ge(est[3][2])
            unsigned char *m = ch == 0 ? bwd_occ : fwd_occ;
            if (!m) continue;
            const float4 v = gather4<kVec>(e3 + ch * hw, s);
            const unsigned char e[4] = {(double)v.x >= 0.6666, (double)v.y >= 0.6666, (double)v.z >= 0.6666, (double)v.w >= 0.6666};
            store4(m + b * hw0 + d, e, n);
        }
    }
}

hipError_t launch_outputs_f32(const float *flow_net, const float *occ, const float *est3, int est3_ch, int B, int fh, int fw, int H0,
                              int W0, double sc_w, double sc_h, float *flow, float *occ_prob, unsigned char *fwd_occ,
                              unsigned char *bwd_occ, hipStream_t s)
{
    if (!flow && !occ_prob && !fwd_occ && !bwd_occ) return hipSuccess;
    const size_t n = (size_t)B * H0 * (((size_t)W0 + kOutPx - 1) / kOutPx);
    // fw == W0: the column map is the identity and every group of 4 source samples 16-byte aligned (fw and the planes' offsets
    // are multiples of 64 floats; the network buffers are 256-byte aligned)
    if (fw == W0)
        hipLaunchKernelGGL(outputs_f32_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, flow_net, occ, est3, est3_ch, B, fh,
                           fw, H0, W0, sc_w, sc_h, flow, occ_prob, fwd_occ, bwd_occ);
    else
        hipLaunchKernelGGL(outputs_f32_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, flow_net, occ, est3, est3_ch, B, fh,
                           fw, H0, W0, sc_w, sc_h, flow, occ_prob, fwd_occ, bwd_occ);
    return hipGetLastError();
}

// 8-bit transport of input planes whose values are all k / 255 (b2f_ctx.h:pack_u8_piece): the same correctly
// rounded division rebuilds the caller's floats bit for bit.  n multiple of 4 not required.
__global__ void unpack_u8_kernel(const unsigned char *in, size_t n, float *out)
{
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 4 <= n && ((uintptr_t)(in + i) & 3) == 0 && ((uintptr_t)(out + i) & 15) == 0) {
        const uchar4 k = *reinterpret_cast<const uchar4 *>(in + i);
        *reinterpret_cast<float4 *>(out + i) = make_float4(__fdiv_rn((float)k.x, 255.0f), __fdiv_rn((float)k.y, 255.0f),
                                                           __fdiv_rn((float)k.z, 255.0f), __fdiv_rn((float)k.w, 255.0f));
    } else {
        for (size_t q = i; q < n && q < i + 4; ++q) out[q] = __fdiv_rn((float)in[q], 255.0f);
    }
}

hipError_t launch_unpack_u8(const unsigned char *in, size_t n, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(unpack_u8_kernel, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, s, in, n, out);
    return hipGetLastError();
}

}  // namespace b2f
