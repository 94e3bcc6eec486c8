// Sequence-mode glue kernels (b2f_forward_sequence_device): the input is T frames, frame-major T x 3 x H x W, and
// triplet b is made of frames (b, b + 1, b + 2).  The siamese pyramid runs once per frame instead of once per
// (triplet, frame) pair; everything from the cost volume on reads the shared pyramid through per-triplet base
// pointers (b2f_api.hip: forward_impl).  Both kernels repeat the arithmetic of their triplet-mode twins in
// b2f_glue.hip operation for operation, so a sequence's outputs are those of its overlapping triplets bit for bit.
// Samples are fp32 (normalized or [0,1]) or bytes whose value is k / 255 (the correctly rounded quotient
// unpack_u8_kernel, b2f_boundary.hip, rebuilds the fp32 frames with): an 8-bit sequence needs no unpack pass.
#include "../../include/b2f.h"
#include "b2f_internal.h"

namespace b2f {

namespace {

__device__ __forceinline__ float sample_value(float v) { return v; }
__device__ __forceinline__ float sample_value(unsigned char k) { return __fdiv_rn((float)k, 255.0f); }

// conv_first_kernel (b2f_glue.hip) with image i at in + i * 3 * H * W: ColorNormalize + nn.SpatialConvolution(3,16,3,3,2,2,1,1)
// + LeakyReLU(0.2) (pwc.lua:58-61).  Block = 256 threads = 8 x 32 output pixels of one frame; the 17 x 65 x 3 input patch is
// normalized once into LDS; weights [tap 27][cout 16] come in as scalar operands.  out = chunk-planar [T][2][H/2*W/2][8].
template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void conv_first_seq_kernel(
    const T *in, int normalize, int H, int W, const float *wt /*27 x 16*/, const float *bias /*16*/, float *out)
{
    constexpr int TH = 8, TW = 32, PH = 2 * TH + 1, PW = 2 * TW + 1;
    __shared__ float patch[3][PH][PW + 1];
    const int Ho = H >> 1, Wo = W >> 1;
    const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
    int bid = blockIdx.x;
    const int tx_i = bid % tiles_x;
    bid /= tiles_x;
    const int ty_i = bid % tiles_y;
    const int img = bid / tiles_y;          // frame
    const int ox0 = tx_i * TW, oy0 = ty_i * TH;
    const int ix0 = 2 * ox0 - 1, iy0 = 2 * oy0 - 1;
    const size_t hw = (size_t)H * W;
    const T *src = in + (size_t)img * 3 * hw;
    // wave w stages patch rows (c, py) = w, w + 4, ... (51 rows = 13 per wave), lane = column 0..63, column 64 by lane 0;
    // all loads of a wave are issued before the first one is used
    {
        const int lane = threadIdx.x & 63;
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        T v[13], v64[13];
        bool ok[13], ok64[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            const int r = wv + 4 * i;
            const int c = r >= 2 * PH ? 2 : (r >= PH ? 1 : 0), py = r - c * PH;
            const int gy = iy0 + py;
            const bool row_ok = r < 3 * PH && gy >= 0 && gy < H;
            const T *rowp = src + (size_t)(row_ok ? c : 0) * hw + (size_t)(row_ok ? gy : 0) * W;
            const int gx = ix0 + lane, gx64 = ix0 + 64;
            ok[i] = row_ok && gx >= 0 && gx < W;
            ok64[i] = row_ok && lane == 0 && gx64 < W;
            v[i] = rowp[ok[i] ? gx : 0];
            v64[i] = rowp[ok64[i] ? gx64 : 0];
        }
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            const int r = wv + 4 * i;
            const int c = r >= 2 * PH ? 2 : (r >= PH ? 1 : 0), py = r - c * PH;
            if (r < 3 * PH) {
                float a = sample_value(v[i]), b = sample_value(v64[i]);
                if (normalize) {
                    a = color_normalize(a, c);
                    b = color_normalize(b, c);
                }
                patch[c][py][lane] = ok[i] ? a : 0.f;    // zero padding of the NORMALIZED image
                if (lane == 0) patch[c][py][64] = ok64[i] ? b : 0.f;
            }
        }
    }
    __syncthreads();
    const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
    float acc[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = bias[o];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float v = patch[c][2 * ty + ky][2 * tx + kx];
                const float *w = wt + ((c * 3 + ky) * 3 + kx) * 16;
#pragma unroll
                for (int o = 0; o < 16; ++o) acc[o] = fmaf(v, w[o], acc[o]);
            }
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy >= Ho || ox >= Wo) return;
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = acc[o] > 0.f ? acc[o] : 0.2f * acc[o];
    const size_t hwo = (size_t)Ho * Wo;
    float *op = out + (size_t)img * hwo * 16 + ((size_t)oy * Wo + ox) * 8;
    *reinterpret_cast<float4 *>(op) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4 *>(op + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    *reinterpret_cast<float4 *>(op + hwo * 8) = make_float4(acc[8], acc[9], acc[10], acc[11]);
    *reinterpret_cast<float4 *>(op + hwo * 8 + 4) = make_float4(acc[12], acc[13], acc[14], acc[15]);
}

// warp_input_planar_kernel (b2f_glue.hip) for the Hard models' est[3] = iws[1][3] (pwc.lua:422-446): the first frame of
// triplet b, frame b of the sequence, normalized on the fly and warped by k * planar flow -> planar B x 3 x H x W.
// The dx / dy fold (here and in warp_input_planar_kernel): a tap past the last column / row is read from the top-left pixel again
// instead of being replaced by 0, so every read stays inside frame b (src[dy + dx] on the last row and column is src[0]).  xl = W - 1
// is reached only through the clamp, with c = W - 1 exactly: wx = 1 and the folded tap's weight 1 - wx is exactly 0, so it adds
// 0 * pixel = 0 like the sampler's zero tap for every FINITE pixel; an Inf / NaN pixel in the last column or row would turn the
// output NaN where the sampler gives Inf (tests/test_gpu_displaced.py runs both kernels through the clamp).
template <typename T>
__global__ void warp_input_seq_kernel(const T *in, int normalize, const float *flow, float k, int B, int H, int W, float *out)
{
    const size_t hw = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * hw) return;
    const size_t b = i / hw, p = i - b * hw;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const float u = flow[(b * 2) * hw + p] * k, v = flow[(b * 2 + 1) * hw + p] * k;
    int xl, yt;
    float wx, wy;
    bhwd_top_left(u + (float)x, W, xl, wx);
    bhwd_top_left(v + (float)y, H, yt, wy);
    const int dx = (xl + 1 <= W - 1) ? 1 : 0, dy = (yt + 1 <= H - 1) ? W : 0;   // weight is 0 when folded
    const float w00 = wx * wy, w01 = (1.f - wx) * wy, w10 = wx * (1.f - wy), w11 = (1.f - wx) * (1.f - wy);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T *src = in + (b * 3 + c) * hw + (size_t)yt * W + xl;
        float tl = sample_value(src[0]), tr = sample_value(src[dx]), bl = sample_value(src[dy]), br = sample_value(src[dy + dx]);
        if (normalize) {
            tl = color_normalize(tl, c); tr = color_normalize(tr, c);
            bl = color_normalize(bl, c); br = color_normalize(br, c);
        }
        out[(b * 3 + c) * hw + p] = w00 * tl + w01 * tr + w10 * bl + w11 * br;
    }
}

}  // namespace

hipError_t launch_conv_first_seq(const void *in, int in_kind, int T, int H, int W, const float *wt, const float *bias, float *out,
                                 hipStream_t s)
{
    const int Ho = H / 2, Wo = W / 2;
    const int tiles = ((Wo + 31) / 32) * ((Ho + 7) / 8);
    const dim3 grid((unsigned)(tiles * T)), block(256);
    if (in_kind == B2F_IN_U8)
        hipLaunchKernelGGL(conv_first_seq_kernel<unsigned char>, grid, block, 0, s, (const unsigned char *)in, 1, H, W, wt, bias, out);
    else
        hipLaunchKernelGGL(conv_first_seq_kernel<float>, grid, block, 0, s, (const float *)in, in_kind == B2F_IN_UNIT ? 1 : 0, H, W,
                           wt, bias, out);
    return hipGetLastError();
}

hipError_t launch_warp_input_seq(const void *in, int in_kind, const float *flow_planar, float k, int B, int H, int W, float *out,
                                 hipStream_t s)
{
    const size_t n = (size_t)B * H * W;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (in_kind == B2F_IN_U8)
        hipLaunchKernelGGL(warp_input_seq_kernel<unsigned char>, grid, block, 0, s, (const unsigned char *)in, 1, flow_planar, k, B, H,
                           W, out);
    else
        hipLaunchKernelGGL(warp_input_seq_kernel<float>, grid, block, 0, s, (const float *)in, in_kind == B2F_IN_UNIT ? 1 : 0,
                           flow_planar, k, B, H, W, out);
    return hipGetLastError();
}

}  // namespace b2f
