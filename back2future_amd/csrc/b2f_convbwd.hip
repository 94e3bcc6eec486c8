// The backward pass of a stride-1 conv layer for gfx950 (MI355X): nn.SpatialConvolution(Ci,Co,3,3,1,1,1,1) [+ nn.LeakyReLU(0.2, true)] :backward
// (pwc.lua:58-65 second conv of a convUnit, :76-85 every decoder layer), DESIGN.md 7.19.  x: B x Ci x H x W, w: Co x Ci x 3 x 3, y: the
// layer's output, gy: the gradient with respect to y.
//
//   g'  = gy * (y > 0 ? 1 : 0.2f)  (LeakyReLU:updateGradInput tests input > 0; the kernels compute y = max(v, 0.2f v), so v > 0 <=> y > 0
//         and the saved OUTPUT is all the layer needs), g' = gy without the activation                                     leaky_mask
//   gx  = conv3x3(g', w~, bias 0, no LeakyReLU), w~[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx]: the forward's own kernels through
//         launch_layer / choose_kernel, nothing of them is edited; the profile row is the forward kernel's
//   gw[co][ci][ky][kx] = sum over (b, oy, ox) of g'[b][co][oy][ox] * x[b][ci][oy + ky - 1][ox + kx - 1], zero padding       conv3x3_gradw
//   gb[co] = sum over (b, oy, ox) of g'[b][co][oy][ox]                                                                      gradb_partials
//   gw and gb are written, not accumulated (Torch after zeroGradParameters).
//
// conv3x3_gradw is a GEMM with M = Co, N = 9 taps x Ci, K = B H W pixels on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain over k):
// the A operand is one VGPR g'[pixel p + (lane >> 5)][co = lane & 31], the B operand one VGPR x[that pixel shifted by the tap][ci = lane & 31],
// the sum index k is the pixel: one MFMA adds two pixels to a 32 co x 32 ci tile of one tap.
//   * the pixels are walked in STRIPS of kGradwBandRows output rows x kGradwStripCols output columns of one image, in the order
//     strip = (image * bands + band) * strips_per_row + column strip, rows then columns inside a strip.  Per strip the block stages in LDS the
//     g' strip and the x strip with a one-pixel halo ((kGradwBandRows + 2) x (kGradwStripCols + 2) pixels, zero outside the map and outside
//     the channel count by masking the load: the address of a masked element is the buffer's base), so one x load serves all nine taps.
//     LDS layout [4-channel group][pixel] of float4 with an odd pixel count per plane: the float4 stores of neighbouring pixels and the
//     one-float operand reads of 32 channels x one pixel are both free of bank conflicts.
//   * block tile = MC x 32 output channels x NC x 32 input channels x 9 taps, MC in {1, 2, 3}, NC in {1, 2}: whichever pads the channel
//     counts least (the choice moves no bit: every element is the same chain over the pixels).  MC x NC waves; a wave owns one 32 x 32
//     tile of every tap: nine independent accumulators (144 registers), ten one-float LDS reads per nine MFMAs.
//   * split of K: the strips are cut into P partials of q = ceil(strips / P0) consecutive strips, P = ceil(strips / q), where
//     P0 = clamp(floor(kGradwRuleCUs * floor(kGradwWavesPerCU / (MC NC)) / output tiles), 1, min(kGradwMaxPartials, strips /
//     kGradwMinStrips)) -- as many blocks as 256 CUs of 8 waves hold at once, so that the launch is one round of equal blocks --: a function
//     of (B, H, W, Ci, Co) alone, not of the device, its CU count or any option but the test option op_gradw_partials (> 0: P0 = that,
//     at most the strip count).  Block (tile, partial) writes its tile of partial sums to the workspace, gradw_reduce adds the
//     partials of an element in index order, gradb_partials / gradw_reduce do the same for gb.  No floating-point atomics anywhere:
//     the same call gives the same bits on any device and in any run.
//   * workspace: P x 9 x Co_pad x Ci_pad floats for gw (Co_pad, Ci_pad: the channel counts rounded up to whole block tiles) and
//     P x Co_pad8 floats for gb (Co rounded up to 8); 128 -> 128 at 4 x 256 x 480: P = 128, 75.5 MB.
//   * longest chain: the most in-map pixels any partial sums (padding pixels add an exact zero); b2f_op_conv3x3_backward_plan reports it
//     with P, and the tests' bound is (longest chain + P + 2) u S.
// Every kernel takes (img_stride, chunk_stride, pix_stride) in floats for x and g' like the forward's kernels: NHWC (chunk 8, pix C) and
// the forward's chunk-planar layout are both expressible.
//
// The stride-2 layers (nn.SpatialConvolution(Ci,Co,3,3,2,2,1,1), the first conv of a convUnit) have entries of their own,
// b2f_op_conv3x3s2_backward[_plan]; b2f_op_conv3x3_backward refuses them.  x and gx are H x W, y, gy and g' Ho x Wo = ((H - 1) / 2 + 1) x
// ((W - 1) / 2 + 1).  leaky_mask, gradb_partials and gradw_reduce are the same kernels on the Ho x Wo map; conv3x3_gradw is instantiated
// with ST = 2: strips of kGradwBandRows x kGradwS2StripCols output pixels, an x strip of 5 x (2 kGradwS2StripCols + 1) input pixels with
// the halo on the low side only, tap (ky, kx) of output pixel (r, j) at x strip pixel (2 r + ky, 2 j + kx), the pixel pair member two
// input pixels on; the ST = 1 instances are the code they were.  gradInput is a transposed convolution no forward kernel computes:
// conv3x3s2_gradx below.
#include "b2f_ctx.h"

#include <cstdio>

namespace b2f {

constexpr int kGradwBandRows = 2;        // output rows of a strip
constexpr int kGradwStripCols = 32;      // output columns of a strip
constexpr int kGradwRuleCUs = 256;       // the split aims at one round of blocks on this many CUs (a constant of the rule, not the device's count)
constexpr int kGradwWavesPerCU = 8;      // ... with this many waves each: 144 accumulator registers leave two waves per SIMD
constexpr int kGradwMinStrips = 8;       // a partial of the rule holds at least this many strips ...
constexpr int kGradwMaxPartials = 256;   // ... and there are at most this many
constexpr int kGradwS2StripCols = 16;    // output columns of a strip of a stride-2 layer (its x strip: 5 x 33 input pixels)
constexpr int kGradxS2Rows = 4;          // conv3x3s2_gradx: output rows of a block's tile of g', one per wave
constexpr int kGradxS2Cols = 32;         // ... and its output columns, the pixel dimension of a wave's MFMA tile
constexpr int kGradxS2Co = 32;           // ... and the output channels staged in LDS at a time

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// element (b, c, q) of a source of leaky_mask: b * img + (c >> 3) * chunk + (c & 7) * ch + q * pix
struct MaskSrc {
    const float *p;
    long img, chunk, ch;
    int pix;
};

// g' in the consumers' layout, channels padded to chunks of 8 with zeros (the gradInput conv multiplies them): thread = (image, chunk,
// pixel, half chunk) writes one float4.  vec: the sources hold the 4 channels of a half chunk contiguously and 16-byte aligned, and C is a
// multiple of 4 (a half chunk is all channels or all padding).  y = nullptr: no activation, g' = gy.
__global__ __launch_bounds__(256) void leaky_mask(MaskSrc gy, MaskSrc y, int C, int B, int hw, int vec, float *out, long out_img, long out_chunk,
                                                  int out_pix)
{
    const int nch = (C + 7) >> 3;
    const size_t total = (size_t)B * nch * hw * 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int hf = (int)(i & 1);
    size_t r = i >> 1;
    const int q = (int)(r % hw);
    r /= hw;
    const int chunk = (int)(r % nch), b = (int)(r / nch);
    const int c0 = chunk * 8 + hf * 4;
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, v = {1.f, 1.f, 1.f, 1.f};
    if (vec) {
        const bool ok = c0 < C;
        const size_t og = ok ? (size_t)b * gy.img + (size_t)chunk * gy.chunk + (size_t)q * gy.pix + hf * 4 : 0;
        const f32x4 lg = *reinterpret_cast<const f32x4 *>(gy.p + og);
        if (ok) g = lg;
        if (y.p) {
            const size_t oy = ok ? (size_t)b * y.img + (size_t)chunk * y.chunk + (size_t)q * y.pix + hf * 4 : 0;
            v = *reinterpret_cast<const f32x4 *>(y.p + oy);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = c0 + j < C;
            const size_t og = ok ? (size_t)b * gy.img + (size_t)chunk * gy.chunk + (size_t)(hf * 4 + j) * gy.ch + (size_t)q * gy.pix : 0;
            const float lg = gy.p[og];
            if (ok) g[j] = lg;
            if (y.p) {
                const size_t oy = ok ? (size_t)b * y.img + (size_t)chunk * y.chunk + (size_t)(hf * 4 + j) * y.ch + (size_t)q * y.pix : 0;
                v[j] = y.p[oy];
            }
        }
    }
    if (y.p) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] : 0.2f * g[j];   // y == 0 takes the slope
    }
    *reinterpret_cast<f32x4 *>(out + (size_t)b * out_img + (size_t)chunk * out_chunk + (size_t)q * out_pix + hf * 4) = g;
}

struct GradwLaunch {
    const float *x;       // chunks of 8 channels, x_chunks of them
    long x_img, x_chunk;
    int x_pix, x_chunks;
    const float *g;       // g', g_chunks chunks
    long g_img, g_chunk;
    int g_pix, g_chunks;
    int H, W;             // the map of g'
    int xH, xW;           // the map of x: H, W at stride 1
    int bands, nsx;       // strips per image column, per image row
    int strips, q;        // all strips; strips per partial
    int n_co_tiles;       // block tiles along Co (blockIdx.x = ci tile * n_co_tiles + co tile)
    int co_pad, ci_pad;   // workspace extents
    float *ws;            // [partial][tap 9][co_pad][ci_pad]
};

// ST: the layer's stride, 1 or 2.  The x strip of an RB x SW strip of g' is (ST (RB - 1) + 3) x (ST (SW - 1) + 3) input pixels from
// (ST oy0 - 1, ST ox0 - 1): a halo on both sides at stride 1, on the low side only at stride 2.
template <int MC, int NC, int ST>
__global__ __launch_bounds__(MC * NC * 64) void conv3x3_gradw(const GradwLaunch p)
{
    constexpr int NTHR = MC * NC * 64;
    constexpr int RB = kGradwBandRows, SW = ST == 1 ? kGradwStripCols : kGradwS2StripCols;
    constexpr int GPIX = RB * SW, XW = ST * (SW - 1) + 3, XPIX = (ST * (RB - 1) + 3) * XW;
    constexpr int GNP = GPIX | 1, XNP = XPIX | 1;             // pixels per LDS plane: odd
    constexpr int G_ITEMS = MC * 8 * GPIX, X_ITEMS = NC * 8 * XPIX;   // float4 items of a strip
    constexpr int G_ITER = (G_ITEMS + NTHR - 1) / NTHR, X_ITER = (X_ITEMS + NTHR - 1) / NTHR;
    static_assert(G_ITEMS % NTHR == 0, "the g' strip is a whole number of passes");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *G = reinterpret_cast<f32x4 *>(smem);               // [MC * 8 planes][GNP]
    f32x4 *X = G + MC * 8 * GNP;                               // [NC * 8 planes][XNP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mc = wave % MC, nc = wave / MC;
    const int n = lane & 31, half = lane >> 5;
    const int cot = blockIdx.x % p.n_co_tiles, cit = blockIdx.x / p.n_co_tiles;
    const int part = blockIdx.y;
    const int s0 = part * p.q, s1 = min(s0 + p.q, p.strips);

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // this lane's operands: channel n of the wave's 32, pixel pair member `half`
    const float *Gf = reinterpret_cast<const float *>(G) + ((mc * 8 + (n >> 2)) * GNP + half) * 4 + (n & 3);
    const float *Xf = reinterpret_cast<const float *>(X) + ((nc * 8 + (n >> 2)) * XNP + half * ST) * 4 + (n & 3);

    for (int s = s0; s < s1; ++s) {
        const int sx = s % p.nsx;
        const int t = s / p.nsx;
        const int band = t % p.bands, img = t / p.bands;
        const int oy0 = band * RB, ox0 = sx * SW;
        const float *gb = p.g + (size_t)img * p.g_img, *xb = p.x + (size_t)img * p.x_img;
        __syncthreads();   // every wave has read the strip before
        // item = (chunk of the tile, pixel, half chunk), half fastest: a lane pair loads the 32 bytes of one pixel's chunk
#pragma unroll
        for (int i = 0; i < G_ITER; ++i) {
            const int idx = tid + i * NTHR;
            const int hf = idx & 1, pix = (idx >> 1) % GPIX, ch = (idx >> 1) / GPIX;
            const int oy = oy0 + pix / SW, ox = ox0 + pix % SW;
            const int chunk = cot * (MC * 4) + ch;
            const bool ok = oy < p.H && ox < p.W && chunk < p.g_chunks;
            const size_t off = ok ? (size_t)chunk * p.g_chunk + (size_t)(oy * p.W + ox) * p.g_pix + hf * 4 : 0;   // masked: the base
            const f32x4 v = *reinterpret_cast<const f32x4 *>(gb + off);
            G[(ch * 2 + hf) * GNP + pix] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll 4
        for (int i = 0; i < X_ITER; ++i) {
            const int idx = tid + i * NTHR;
            const bool in = (X_ITEMS % NTHR == 0) || idx < X_ITEMS;
            const int hf = idx & 1, pix = (idx >> 1) % XPIX, ch = min((idx >> 1) / XPIX, NC * 4 - 1);
            const int iy = ST * oy0 - 1 + pix / XW, ix = ST * ox0 - 1 + pix % XW;
            const int chunk = cit * (NC * 4) + ch;
            const bool ok = in && iy >= 0 && iy < p.xH && ix >= 0 && ix < p.xW && chunk < p.x_chunks;
            const size_t off = ok ? (size_t)chunk * p.x_chunk + (size_t)(iy * p.xW + ix) * p.x_pix + hf * 4 : 0;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + off);
            if (in) X[(ch * 2 + hf) * XNP + pix] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll 4
            for (int j = 0; j < SW / 2; ++j) {
                const float a = Gf[(r * SW + 2 * j) * 4];
                const float *xp = Xf + ST * (r * XW + 2 * j) * 4;
                float b[9];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) b[tap] = xp[((tap / 3) * XW + tap % 3) * 4];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[tap], acc[tap], 0, 0, 0);
            }
        }
    }
    // C/D layout: column = lane & 31 (ci), row = (r & 3) + 8 * (r >> 2) + 4 * half (co); always inside the padded workspace
    const int ci = (cit * NC + nc) * 32 + n;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = (cot * MC + mc) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            p.ws[(((size_t)part * 9 + tap) * p.co_pad + co) * p.ci_pad + ci] = acc[tap][r];
        }
}

// gb's partial sums: block (chunk of 8 channels, partial), thread = (sub 0..7, channel): thread `sub` adds the strip positions
// sub, sub + 8, .. of every strip of the partial in order, then thread 0 of a channel adds the eight sums in order.  wsb: [partial][chunks * 8]
template <int SW>
__global__ __launch_bounds__(64) void gradb_partials(const GradwLaunch p, float *wsb)
{
    constexpr int RB = kGradwBandRows;
    __shared__ float sums[64];
    const int ch = threadIdx.x & 7, sub = threadIdx.x >> 3;
    const int chunk = blockIdx.x, part = blockIdx.y;
    const int s0 = part * p.q, s1 = min(s0 + p.q, p.strips);
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) {
        const int sx = s % p.nsx;
        const int t = s / p.nsx;
        const int band = t % p.bands, img = t / p.bands;
        const float *gb = p.g + (size_t)img * p.g_img + (size_t)chunk * p.g_chunk + ch;
#pragma unroll
        for (int k = 0; k < RB * SW / 8; ++k) {
            const int pix = sub + 8 * k;
            const int oy = band * RB + pix / SW, ox = sx * SW + pix % SW;
            const bool ok = oy < p.H && ox < p.W;
            const float v = gb[ok ? (size_t)(oy * p.W + ox) * p.g_pix : 0];
            acc = acc + (ok ? v : 0.f);
        }
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    if (sub == 0) {
        float a = sums[ch];
#pragma unroll
        for (int k = 1; k < 8; ++k) a = a + sums[k * 8 + ch];
        wsb[(size_t)part * (gridDim.x * 8) + chunk * 8 + ch] = a;
    }
}

// gw[co][ci][tap] = ws[0] + ws[1] + .. + ws[P - 1] in that order (thread = (tap, co, ci), ci fastest: coalesced reads), then gb the same
// way from wsb; gw / gb may be null
__global__ __launch_bounds__(256) void gradw_reduce(const float *ws, const float *wsb, int P, int Co, int Ci, int co_pad, int ci_pad, int cob_pad,
                                                    float *gw, float *gb)
{
    const size_t nw = gw ? (size_t)9 * Co * Ci : 0;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        const int ci = (int)(i % Ci);
        const size_t r = i / Ci;
        const int co = (int)(r % Co), tap = (int)(r / Co);
        const size_t plane = (size_t)9 * co_pad * ci_pad;
        const float *src = ws + ((size_t)tap * co_pad + co) * ci_pad + ci;
        float a = src[0];
        for (int k = 1; k < P; ++k) a = a + src[(size_t)k * plane];
        gw[((size_t)co * Ci + ci) * 9 + tap] = a;
    } else if (gb && i - nw < (size_t)Co) {
        const int co = (int)(i - nw);
        float a = wsb[co];
        for (int k = 1; k < P; ++k) a = a + wsb[(size_t)k * cob_pad + co];
        gb[co] = a;
    }
}

struct GradxS2Launch {
    const float *g;       // g' on the Ho x Wo map, g_chunks chunks of 8 channels
    long g_img, g_chunk;
    int g_pix, g_chunks;
    const float *wp;      // [tap 9][co_pad][ci_pad]: w[co][ci][tap], zero in the padding
    int co_pad, ci_pad;   // multiples of kGradxS2Co and of 32
    int Ho, Wo, H, W;     // the maps of g' and of gx
    int tiles_x, tiles_y; // tiles of kGradxS2Rows x kGradxS2Cols pixels of g' per image (blockIdx.x = (image * tiles_y + ty) * tiles_x + tx)
    float *out;           // gx, out_chunks chunks of 8 channels
    long out_img, out_chunk;
    int out_pix, out_chunks;
};

// gradInput of a stride-2 layer, a transposed convolution: the pixel (2 oy + py, 2 ox + px) of gx takes, by its parity class (py, px),
//   (0, 0): g'(oy, ox) w[1][1]                                  (0, 1): g'(oy, ox + 1) w[1][0] + g'(oy, ox) w[1][2]
//   (1, 0): g'(oy + 1, ox) w[0][1] + g'(oy, ox) w[2][1]         (1, 1): g'(oy + 1, ox + 1) w[0][0] + g'(oy + 1, ox) w[0][2]
//                                                                       + g'(oy, ox + 1) w[2][0] + g'(oy, ox) w[2][2]
// summed over co: nine taps per 2 x 2 pixels of gx, the forward layer's MAC count; no zero-inserted g' exists anywhere.
// A GEMM per class with M = ci, N = pixel, K = co on v_mfma_f32_32x32x2_f32: A = one VGPR w[tap][co = k + (lane >> 5)][ci = lane & 31],
// B = one VGPR g'[co = k + (lane >> 5)][row, column + (lane & 31)] at the class's neighbour.  Block = 4 waves = 32 input channels x a tile
// of kGradxS2Rows x kGradxS2Cols pixels of g' of one image; wave v owns row v of the tile and the four classes' 32 ci x 32 pixel
// accumulators (64 registers); per pair of output channels it reads four B and nine A operands and issues nine MFMAs, a class's taps in
// the order above, the pairs in the order of co: every element of gx is one fmaf chain over (co pair, tap, co of the pair).
// Per kGradxS2Co output channels the block stages in LDS g' of the tile with one halo row below and one halo column right, zero
// outside the map and the channel count by masking the load, as [co][172 floats: 5 x 33 pixels + 7] -- the operand read of 32 pixels
// and the four one-float stores of a loaded float4 (lane pairs 4 x 172 = 16 mod 32 banks apart) are free of bank conflicts -- and the
// weights as [tap][co][32 ci]: 22 016 + 36 864 bytes, two blocks per CU; 78 + 64 registers, no scratch.  D: a lane holds ci = 8 (r >> 2) + 4 (lane >> 5) + (r & 3) of
// pixel lane & 31: one float4 store per half chunk, masked at iy >= H and ix >= W (the odd / odd pixel past an odd H or W does not exist).
__global__ __launch_bounds__(256) void conv3x3s2_gradx(const GradxS2Launch p)
{
    constexpr int TH = kGradxS2Rows, TW = kGradxS2Cols, KC = kGradxS2Co;
    constexpr int GW = TW + 1, GPIX = (TH + 1) * GW, GP = 172;
    constexpr int G_ITEMS = (KC / 8) * GPIX * 2, W_ITEMS = 9 * KC * 8;   // float4 items
    static_assert(GP >= GPIX && GP % 8 == 4, "a row of the g' tile holds its pixels; 4 rows are 16 banks apart");
    static_assert(TH == 4 && TW == 32 && KC % 8 == 0 && W_ITEMS % 256 == 0, "one wave per row, 32 pixels per MFMA tile");
    __shared__ float Gs[KC * GP];
    __shared__ __attribute__((aligned(16))) float Ws[9 * KC * 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, half = lane >> 5;
    const int tx = blockIdx.x % p.tiles_x, t = blockIdx.x / p.tiles_x;
    const int ty = t % p.tiles_y, img = t / p.tiles_y;
    const int cit = blockIdx.y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const float *gb = p.g + (size_t)img * p.g_img;

    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    const float *gr = Gs + half * GP + wave * GW + n;
    const float *wr = Ws + half * 32 + n;
    const bool row_in = oy0 + wave < p.Ho;   // wave-uniform

    for (int k0 = 0; k0 < p.co_pad; k0 += KC) {
        __syncthreads();   // every wave has read the channels before
        // item = (chunk, pixel, half chunk), half fastest: a lane pair loads the 32 bytes of one pixel's chunk
        for (int idx = tid; idx < G_ITEMS; idx += 256) {
            const int hf = idx & 1, pix = (idx >> 1) % GPIX, ch = (idx >> 1) / GPIX;
            const int oy = oy0 + pix / GW, ox = ox0 + pix % GW;
            const int chunk = k0 / 8 + ch;
            const bool ok = oy < p.Ho && ox < p.Wo && chunk < p.g_chunks;
            const size_t off = ok ? (size_t)chunk * p.g_chunk + (size_t)(oy * p.Wo + ox) * p.g_pix + hf * 4 : 0;   // masked: the base
            const f32x4 v = *reinterpret_cast<const f32x4 *>(gb + off);
            float *d = Gs + (ch * 8 + hf * 4) * GP + pix;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j * GP] = ok ? v[j] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < W_ITEMS / 256; ++i) {
            const int idx = tid + i * 256;
            const int c4 = idx & 7, row = idx >> 3;   // row = tap * KC + co of the stage
            const int tap = row / KC, k = row % KC;
            *reinterpret_cast<f32x4 *>(Ws + row * 32 + c4 * 4) =
                *reinterpret_cast<const f32x4 *>(p.wp + ((size_t)tap * p.co_pad + k0 + k) * p.ci_pad + cit * 32 + c4 * 4);
        }
        __syncthreads();
        if (row_in) {
#pragma unroll 2
            for (int k = 0; k < KC; k += 2) {
                const float b00 = gr[k * GP], b01 = gr[k * GP + 1], b10 = gr[k * GP + GW], b11 = gr[k * GP + GW + 1];
                float a[9];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) a[tap] = wr[(tap * KC + k) * 32];
                // the four classes interleaved: no MFMA reads the accumulator the one before it writes
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b11, acc[3], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4], b00, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b01, acc[1], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b10, acc[3], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b10, acc[2], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[5], b00, acc[1], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[6], b01, acc[3], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[7], b00, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[8], b00, acc[3], 0, 0, 0);
            }
        }
    }
    // C/D layout: column = lane & 31 (pixel), row = (r & 3) + 8 * (r >> 2) + 4 * half (ci): the half chunk `half` of chunk r >> 2
    const int oy = oy0 + wave, ox = ox0 + n;
    float *ob = p.out + (size_t)img * p.out_img + half * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int iy = 2 * oy + (c >> 1), ix = 2 * ox + (c & 1);
        if (!row_in || iy >= p.H || ix >= p.W) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int chunk = cit * 4 + q;
            if (chunk >= p.out_chunks) continue;
            const f32x4 v = {acc[c][4 * q], acc[c][4 * q + 1], acc[c][4 * q + 2], acc[c][4 * q + 3]};
            *reinterpret_cast<f32x4 *>(ob + (size_t)chunk * p.out_chunk + (size_t)(iy * p.W + ix) * p.out_pix) = v;
        }
    }
}

// The split and the tiles of a call: everything from (B, Ci, H, W, Co) and the forced partial count (0 = the rule); no HIP call
struct GradwPlan {
    int mc, nc;                  // 32-channel tiles per block along Co, Ci
    int n_co_tiles, n_ci_tiles;
    int co_pad, ci_pad;
    int bands, nsx, strips, q, P;
    long long longest_chain;     // the most in-map pixels a partial sums
};

// tiles per block out of 1 .. most that pad `n32` tiles of 32 channels least; the larger block on a tie
int pick_tiles(int n32, int most)
{
    int best = 1, pad = n32;
    for (int m = 2; m <= most; ++m) {
        const int pm = (n32 + m - 1) / m * m;
        if (pm <= pad) { best = m; pad = pm; }
    }
    return best;
}

// H, W: the map of g'; sw: the strip's columns (kGradwStripCols, or kGradwS2StripCols for a stride-2 layer)
GradwPlan gradw_plan(int B, int Ci, int H, int W, int Co, int forced, int sw = kGradwStripCols)
{
    GradwPlan g{};
    g.mc = pick_tiles((Co + 31) / 32, 3);
    g.nc = pick_tiles((Ci + 31) / 32, 2);
    g.n_co_tiles = ((Co + 31) / 32 + g.mc - 1) / g.mc;
    g.n_ci_tiles = ((Ci + 31) / 32 + g.nc - 1) / g.nc;
    g.co_pad = g.n_co_tiles * g.mc * 32;
    g.ci_pad = g.n_ci_tiles * g.nc * 32;
    g.bands = (H + kGradwBandRows - 1) / kGradwBandRows;
    g.nsx = (W + sw - 1) / sw;
    g.strips = B * g.bands * g.nsx;
    const int tiles = g.n_co_tiles * g.n_ci_tiles;
    int p0;
    if (forced > 0) p0 = std::min(forced, g.strips);
    else {
        // blocks of MC x NC waves that kGradwRuleCUs CUs of kGradwWavesPerCU waves hold at once: at most that many blocks, so one round
        const int at_once = kGradwRuleCUs * std::max(1, kGradwWavesPerCU / (g.mc * g.nc));
        p0 = std::max(1, std::min({at_once / tiles, kGradwMaxPartials, g.strips / kGradwMinStrips}));
    }
    g.q = (g.strips + p0 - 1) / p0;
    g.P = (g.strips + g.q - 1) / g.q;
    for (int part = 0; part < g.P; ++part) {
        long long n = 0;
        for (int s = part * g.q; s < std::min((part + 1) * g.q, g.strips); ++s) {
            const int sx = s % g.nsx, band = (s / g.nsx) % g.bands;
            n += (long long)std::min(kGradwBandRows, H - band * kGradwBandRows) * std::min(sw, W - sx * sw);
        }
        g.longest_chain = std::max(g.longest_chain, n);
    }
    return g;
}

template <int MC, int NC, int ST>
hipError_t launch_gradw_t(const GradwLaunch &L, int n_ci_tiles, int P, hipStream_t s)
{
    constexpr int RB = kGradwBandRows, SW = ST == 1 ? kGradwStripCols : kGradwS2StripCols;
    constexpr int GNP = (RB * SW) | 1, XNP = ((ST * (RB - 1) + 3) * (ST * (SW - 1) + 3)) | 1;
    // the largest, MC = 3 and NC = 2: 60 032 bytes at stride 1, 54 912 at stride 2
    constexpr size_t lds = sizeof(f32x4) * (MC * 8 * GNP + NC * 8 * XNP);
    static LdsOnce once;   // one per template instance
    if (hipError_t e = once.ensure(reinterpret_cast<const void *>(&conv3x3_gradw<MC, NC, ST>), (int)lds)) return e;
    hipLaunchKernelGGL((conv3x3_gradw<MC, NC, ST>), dim3((unsigned)(L.n_co_tiles * n_ci_tiles), (unsigned)P), dim3(MC * NC * 64), lds, s, L);
    return hipGetLastError();
}

template <int ST>
hipError_t launch_gradw(const GradwPlan &g, const GradwLaunch &L, hipStream_t s)
{
    switch (g.mc * 10 + g.nc) {
        case 11: return launch_gradw_t<1, 1, ST>(L, g.n_ci_tiles, g.P, s);
        case 12: return launch_gradw_t<1, 2, ST>(L, g.n_ci_tiles, g.P, s);
        case 21: return launch_gradw_t<2, 1, ST>(L, g.n_ci_tiles, g.P, s);
        case 22: return launch_gradw_t<2, 2, ST>(L, g.n_ci_tiles, g.P, s);
        case 31: return launch_gradw_t<3, 1, ST>(L, g.n_ci_tiles, g.P, s);
        case 32: return launch_gradw_t<3, 2, ST>(L, g.n_ci_tiles, g.P, s);
    }
    return hipErrorInvalidValue;
}

// a launch on s as the row `name` of b2f_profile_read
template <class Launch>
int timed(b2f_ctx *c, hipStream_t s, const char *name, Launch launch)
{
    ProfEvent pe;
    const bool on = prof_open(c, s, name, &pe);
    const hipError_t e = launch();
    if (on) prof_close(c, s, pe);
    HIPCHK(e);
    return 0;
}

// planar [image][C][hw] -> chunk-planar [image][(C + 7) / 8][hw][8], zero padding
void planar_to_cp8_host(const float *src, size_t images, int C, size_t hw, float *dst)
{
    const size_t Cp = (size_t)(C + 7) / 8 * 8;
    std::fill(dst, dst + images * Cp * hw, 0.f);
    for (size_t b = 0; b < images; ++b)
        for (int ch = 0; ch < C; ++ch) {
            const float *s = src + (b * C + ch) * hw;
            float *d = dst + (b * Cp + (size_t)(ch / 8) * 8) * hw + (ch & 7);
            for (size_t i = 0; i < hw; ++i) d[i * 8] = s[i];
        }
}

// the sizes the entries accept: every staged tensor at most 2^28 floats, a map below 2^24 pixels
const char *size_refusal(int B, int Ci, int H, int W, int Co)
{
    if (B <= 0) return "B must be positive";
    if (Ci <= 0) return "Ci must be positive";
    if (H <= 0) return "H must be positive";
    if (W <= 0) return "W must be positive";
    if (Co <= 0) return "Co must be positive";
    if ((long long)H * W >= (1LL << 24) || (long long)B * H * W * (std::max(Ci, Co) + 7) > (1LL << 28) || (long long)Ci * Co > (1LL << 22))
        return "B, Ci, H, W, Co: too large for an op entry (B H W max(Ci, Co) <= 2^28, H W < 2^24, Ci Co <= 2^22)";
    return nullptr;
}

}  // namespace
}  // namespace b2f

using namespace b2f;

namespace {

// the argument checks both backward entries share, in the order they are made; nullptr: none applies
const char *argument_refusal(const float *x, const float *w, const float *y, const float *grad_y, int leaky, const float *grad_x,
                             const float *grad_w, const float *grad_b)
{
    if (!x) return "x is null";
    if (!w) return "w is null";
    if (!grad_y) return "grad_y is null";
    if (leaky && !y) return "y is null: with leaky the layer's output is needed";
    if (!grad_x && !grad_w && !grad_b) return "grad_x, grad_w and grad_b are all null: nothing to compute";
    return nullptr;
}

// The body of both backward entries behind their argument checks.  ST: the layer's stride; H x W: the map of x and gx; y, gy and g' are
// Ho x Wo = ((H - 1) / ST + 1) x ((W - 1) / ST + 1).
template <int ST>
int run_backward(b2f_ctx *c, const char *entry, const float *x, int B, int Ci, int H, int W, const float *w, int Co, int leaky, const float *y,
                 const float *grad_y, int layout, float *grad_x, float *grad_w, float *grad_b)
{
    OpStage st(c, entry);
    CHK(st.begin());
    hipStream_t s = c->stream;
    const int Ho = (H - 1) / ST + 1, Wo = (W - 1) / ST + 1;
    const size_t hw = (size_t)H * W, hwo = (size_t)Ho * Wo;
    const int xch = (Ci + kCK - 1) / kCK, gch = (Co + kCK - 1) / kCK, Cip = xch * kCK, Cop = gch * kCK;
    const size_t nx = (size_t)B * Ci * hw, ny = (size_t)B * Co * hwo, nxp = (size_t)B * Cip * hw, nyp = (size_t)B * Cop * hwo;
    const size_t nw = (size_t)Co * Ci * 9;
    // strides of a C-channel tensor of n pixels in the entry's layout: NHWC on padded channels, or chunk-planar
    auto strides = [&](int Cpad, size_t n, long *img, long *chunk, int *pix) {
        *img = (long)(n * Cpad);
        if (layout == 0) { *chunk = 8; *pix = Cpad; }
        else { *chunk = (long)(n * 8); *pix = 8; }
    };
    long x_img, x_chunk, g_img, g_chunk;
    int x_pix, g_pix;
    strides(Cip, hw, &x_img, &x_chunk, &x_pix);
    strides(Cop, hwo, &g_img, &g_chunk, &g_pix);

    // ---- g' = the masked output gradient, once, in the layout both consumers read ----
    float *dgy, *dyy = nullptr, *dg;
    MaskSrc sg{}, sy{};
    int vec = 0;
    if (layout == 0) {   // the caller's planar tensors, read through their strides
        CHK(st.in(grad_y, ny, "grad_y", &dgy));
        if (leaky) CHK(st.in(y, ny, "y", &dyy));
        sg = {dgy, (long)(hwo * Co), (long)(hwo * 8), (long)hwo, 1};
        sy = {dyy, (long)(hwo * Co), (long)(hwo * 8), (long)hwo, 1};
    } else {             // chunk-planar, as a graph walk would hold them
        std::vector<float> host(nyp);
        planar_to_cp8_host(grad_y, (size_t)B, Co, hwo, host.data());
        CHK(st.in(host.data(), nyp, "grad_y", &dgy));
        if (leaky) {
            planar_to_cp8_host(y, (size_t)B, Co, hwo, host.data());
            CHK(st.in(host.data(), nyp, "y", &dyy));
        }
        sg = {dgy, (long)(hwo * Cop), (long)(hwo * 8), 1, 8};
        sy = {dyy, (long)(hwo * Cop), (long)(hwo * 8), 1, 8};
        vec = Co % 4 == 0;
    }
    CHK(st.out(nyp, "masked grad_y", &dg));
    float *dx = nullptr;
    if (grad_w) {
        if (layout == 0) {
            float *dpl;
            CHK(st.in(x, nx, "x planar", &dpl)); CHK(st.out(nxp, "x", &dx));
            HIPCHK(launch_planar_to_nhwc(dpl, Ci, B, H, W, dx, Cip, s));
        } else {
            std::vector<float> host(nxp);
            planar_to_cp8_host(x, (size_t)B, Ci, hw, host.data());
            CHK(st.in(host.data(), nxp, "x", &dx));
        }
    }
    CHK(timed(c, s, "convbwd_mask", [&] {
        const size_t total = (size_t)B * gch * hwo * 2;
        hipLaunchKernelGGL(leaky_mask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sg, sy, Co, B, (int)hwo, vec, dg, g_img, g_chunk, g_pix);
        return hipGetLastError();
    }));

    // ---- gradInput: the forward's kernels on (g', w~), packed as b2f_op_conv3x3 packs a layer ----
    //      (stride 2: conv3x3s2_gradx on a [tap][co][ci] packing, gx in the layout's strides on padded channels) ----
    float *dgx = nullptr, *dgxp = nullptr;
    if (grad_x && ST == 2) {
        GradxS2Launch L{};
        L.co_pad = (Co + kGradxS2Co - 1) / kGradxS2Co * kGradxS2Co;
        L.ci_pad = (Ci + 31) / 32 * 32;
        std::vector<float> wpk((size_t)9 * L.co_pad * L.ci_pad, 0.f);
        for (int co = 0; co < Co; ++co)
            for (int ci = 0; ci < Ci; ++ci)
                for (int t = 0; t < 9; ++t) wpk[((size_t)t * L.co_pad + co) * L.ci_pad + ci] = w[((size_t)co * Ci + ci) * 9 + t];
        float *dw;
        CHK(st.in(wpk.data(), wpk.size(), "weights by tap", &dw));
        CHK(st.out(nxp, "grad_x", &dgx)); CHK(st.out(nx, "grad_x planar", &dgxp));
        L.g = dg; L.g_img = g_img; L.g_chunk = g_chunk; L.g_pix = g_pix; L.g_chunks = gch;
        L.wp = dw;
        L.Ho = Ho; L.Wo = Wo; L.H = H; L.W = W;
        L.tiles_x = (Wo + kGradxS2Cols - 1) / kGradxS2Cols; L.tiles_y = (Ho + kGradxS2Rows - 1) / kGradxS2Rows;
        L.out = dgx; L.out_img = x_img; L.out_chunk = x_chunk; L.out_pix = x_pix; L.out_chunks = xch;
        CHK(timed(c, s, "convbwd_gradx_s2", [&] {
            hipLaunchKernelGGL(conv3x3s2_gradx, dim3((unsigned)(B * L.tiles_y * L.tiles_x), (unsigned)(L.ci_pad / 32)), dim3(256), 0, s, L);
            return hipGetLastError();
        }));
        if (layout == 0) HIPCHK(launch_nhwc_to_planar(dgx, Cip, Ci, B, H, W, dgxp, s));
        else HIPCHK(launch_cp8_to_planar(dgx, Ci, B, H, W, dgxp, s));
    } else if (grad_x) {
        std::vector<float> wt(nw), zero((size_t)Ci, 0.f);
        for (int co = 0; co < Co; ++co)
            for (int ci = 0; ci < Ci; ++ci)
                for (int t = 0; t < 9; ++t) wt[((size_t)ci * Co + co) * 9 + (8 - t)] = w[((size_t)co * Ci + ci) * 9 + t];   // rotated by 180 degrees, transposed
        PackedConv p;
        p.cout = Ci;
        p.chunks[0] = gch;
        p.base = base_kernel(Co, Ci, true, false);
        KernelOpts o = *c;   // the rule of b2f_op_conv3x3 (b2f_ops.hip), unchanged
        o.adaptive_kernels = 0;
        o.wino4_min_pixels = o.wino_split_pixels = (c->op_wino_split && Ci > 32) ? 0x7fffffff : 0;
        size_t npk = 0;
        place_packings(p, true, o, &npk);
        std::vector<float> wpk(npk, 0.f);
        fill_packings(p, wt.data(), zero.data(), Co, nullptr, wpk.data());
        float *dw;
        CHK(st.in(wpk.data(), npk, "rotated weights", &dw));
        const size_t ngx = layout == 0 ? nx : nxp;
        CHK(st.out(ngx, "grad_x", &dgx)); CHK(st.out(nx, "grad_x planar", &dgxp));
        ConvLaunch L{};
        L.seg[0] = {dg, g_img, g_chunk, g_pix, 0};
        L.out = dgx;
        if (layout == 0) { L.out_img_stride = (long)(hw * Ci); L.out_chunk_stride = 8; L.out_pix_stride = Ci; }
        else { L.out_img_stride = x_img; L.out_chunk_stride = x_chunk; L.out_pix_stride = x_pix; }
        L.H = H; L.W = W; L.stride = 1; L.nimg = B; L.leaky = 0;
        CHK(launch_layer(c, s, true, p, dw, o, 0, L));   // the profile row names the forward kernel that ran
        if (layout == 0) HIPCHK(launch_nhwc_to_planar(dgx, Ci, Ci, B, H, W, dgxp, s));
        else HIPCHK(launch_cp8_to_planar(dgx, Ci, B, H, W, dgxp, s));
    }

    // ---- gradWeight and gradBias: partial sums per (tile, partial), then the partials in index order ----
    float *dgw = nullptr, *dgb = nullptr;
    if (grad_w || grad_b) {
        constexpr int SW = ST == 1 ? kGradwStripCols : kGradwS2StripCols;
        const GradwPlan g = gradw_plan(B, Ci, Ho, Wo, Co, c->op_gradw_partials, SW);
        GradwLaunch L{};
        L.x = dx; L.x_img = x_img; L.x_chunk = x_chunk; L.x_pix = x_pix; L.x_chunks = xch;
        L.g = dg; L.g_img = g_img; L.g_chunk = g_chunk; L.g_pix = g_pix; L.g_chunks = gch;
        L.H = Ho; L.W = Wo; L.xH = H; L.xW = W; L.bands = g.bands; L.nsx = g.nsx; L.strips = g.strips; L.q = g.q;
        L.n_co_tiles = g.n_co_tiles; L.co_pad = g.co_pad; L.ci_pad = g.ci_pad;
        float *ws = nullptr, *wsb = nullptr;
        if (grad_w) { CHK(st.out((size_t)g.P * 9 * g.co_pad * g.ci_pad, "gradw partials", &ws)); CHK(st.out(nw, "grad_w", &dgw)); }
        if (grad_b) { CHK(st.out((size_t)g.P * Cop, "gradb partials", &wsb)); CHK(st.out((size_t)Co, "grad_b", &dgb)); }
        L.ws = ws;
        CHK(timed(c, s, "convbwd_gradw", [&] {
            if (grad_w)
                if (hipError_t e = launch_gradw<ST>(g, L, s)) return e;
            if (grad_b) hipLaunchKernelGGL(gradb_partials<SW>, dim3((unsigned)gch, (unsigned)g.P), dim3(64), 0, s, L, wsb);
            return hipGetLastError();
        }));
        CHK(timed(c, s, "convbwd_reduce", [&] {
            const size_t total = (grad_w ? nw : 0) + (grad_b ? (size_t)Co : 0);
            hipLaunchKernelGGL(gradw_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws, wsb, g.P, Co, Ci, g.co_pad, g.ci_pad, Cop, dgw, dgb);
            return hipGetLastError();
        }));
    }
    CHK(st.finish());
    if (grad_x) CHK(st.get(grad_x, dgxp, nx));
    if (grad_w) CHK(st.get(grad_w, dgw, nw));
    if (grad_b) CHK(st.get(grad_b, dgb, (size_t)Co));
    return 0;
}

}  // namespace

extern "C" {

int b2f_op_conv3x3_backward_plan(b2f_ctx *c, int B, int Ci, int H, int W, int Co, int *partials, long long *longest_chain) try
{
    const std::string fn = "b2f_op_conv3x3_backward_plan: ";
    if (!c) return api_fail(fn + "ctx is null");
    if (const char *why = size_refusal(B, Ci, H, W, Co)) return api_fail(fn + why);
    const GradwPlan g = gradw_plan(B, Ci, H, W, Co, c->op_gradw_partials);
    if (partials) *partials = g.P;
    if (longest_chain) *longest_chain = g.longest_chain;
    return 0;
}
B2F_CATCH("b2f_op_conv3x3_backward_plan")

int b2f_op_conv3x3_backward(b2f_ctx *c, const float *x, int B, int Ci, int H, int W, const float *w, int Co, int stride, int leaky, const float *y,
                            const float *grad_y, int layout, float *grad_x, float *grad_w, float *grad_b) try
{
    const std::string fn = "b2f_op_conv3x3_backward: ";
    if (!c) return api_fail(fn + "ctx is null");
    if (const char *why = argument_refusal(x, w, y, grad_y, leaky, grad_x, grad_w, grad_b)) return api_fail(fn + why);
    if (stride != 1) return api_fail(fn + "stride must be 1 (the stride-2 layers: b2f_op_conv3x3s2_backward)");
    if (layout != 0 && layout != 1) return api_fail(fn + "layout must be 0 (NHWC strides) or 1 (chunk-planar)");
    if (const char *why = size_refusal(B, Ci, H, W, Co)) return api_fail(fn + why);
    return run_backward<1>(c, __func__, x, B, Ci, H, W, w, Co, leaky, y, grad_y, layout, grad_x, grad_w, grad_b);
}
B2F_CATCH("b2f_op_conv3x3_backward")

int b2f_op_conv3x3s2_backward_plan(b2f_ctx *c, int B, int Ci, int H, int W, int Co, int *partials, long long *longest_chain) try
{
    const std::string fn = "b2f_op_conv3x3s2_backward_plan: ";
    if (!c) return api_fail(fn + "ctx is null");
    if (const char *why = size_refusal(B, Ci, H, W, Co)) return api_fail(fn + why);
    const GradwPlan g = gradw_plan(B, Ci, (H - 1) / 2 + 1, (W - 1) / 2 + 1, Co, c->op_gradw_partials, kGradwS2StripCols);
    if (partials) *partials = g.P;
    if (longest_chain) *longest_chain = g.longest_chain;
    return 0;
}
B2F_CATCH("b2f_op_conv3x3s2_backward_plan")

int b2f_op_conv3x3s2_backward(b2f_ctx *c, const float *x, int B, int Ci, int H, int W, const float *w, int Co, int leaky, const float *y,
                              const float *grad_y, int layout, float *grad_x, float *grad_w, float *grad_b) try
{
    const std::string fn = "b2f_op_conv3x3s2_backward: ";
    if (!c) return api_fail(fn + "ctx is null");
    if (const char *why = argument_refusal(x, w, y, grad_y, leaky, grad_x, grad_w, grad_b)) return api_fail(fn + why);
    if (layout != 0 && layout != 1) return api_fail(fn + "layout must be 0 (NHWC strides) or 1 (chunk-planar)");
    if (const char *why = size_refusal(B, Ci, H, W, Co)) return api_fail(fn + why);
    return run_backward<2>(c, __func__, x, B, Ci, H, W, w, Co, leaky, y, grad_y, layout, grad_x, grad_w, grad_b);
}
B2F_CATCH("b2f_op_conv3x3s2_backward")

}  // extern "C"
