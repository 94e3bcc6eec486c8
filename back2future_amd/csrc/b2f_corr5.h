// What the persistent "unit" forms of the warp + cost volume share: stage geometry and LDS layout (namespace v5), the profiling
// switches, sampling records, tap gather and blend, the reference-tile DMA, the tile-direction queue and the persistent launcher.
// Used by b2f_corr5.hip (variants 5 and 7, with b2f_corr5_loop.inc) and by the role-specialised experiment kernel (variant 6,
// tools/experiments/csrc/b2f_corr6.hip).  What only variants 5 and 7 use stays in b2f_corr5.hip.
#pragma once
#include "b2f_internal.h"

#include <climits>
#include <cstdio>

namespace b2f {

namespace v5 {
constexpr int R = 4;
constexpr int TH = 8, TW = 16;                 // output tile
constexpr int HH = TH + 2 * R, HW = TW + 2 * R;   // 16 x 24 halo
constexpr int NHP = HH * HW;                   // 384 halo pixels
constexpr int PLN = NHP + 4;                   // float4 per k4 plane of the warped halo: = 4 (mod 8), so that the lane pair (pixel,
                                               // k4 even | odd) of the blend writes distinct LDS banks
constexpr int NK4 = 4;                         // float4 planes of a stage (16 channels)
constexpr int NCC = NK4 / 2;                   // 8-channel chunks of a stage
constexpr int CGC = 4 * NK4;                   // channels of a stage
constexpr int WR = 20, WC = 28;                // source window: rows x columns
constexpr int WPX = WR * WC;
constexpr int WIN_F4 = NCC * WPX * 2;          // float4 of a window buffer, layout [chunk][row][col][16-byte half]: 2 240
constexpr int WPIECES = WIN_F4 / 64;           // 1-KB LDS-DMA pieces per window: 35
static_assert(WIN_F4 % 64 == 0, "window = whole DMA pieces");
constexpr int NTHR = 768;
constexpr int NUNIT = 10;
constexpr int HALO_F4 = NK4 * PLN;
constexpr int REF_F4 = NK4 * TH * TW;
constexpr int NREC = 3;                        // sampling-record buffers (tile-directions alive at once)
constexpr int OFF_WIN = 0, OFF_HALO = OFF_WIN + 2 * WIN_F4, OFF_REF = OFF_HALO + 2 * HALO_F4, OFF_REC = OFF_REF + 2 * REF_F4,
              OFF_BB = OFF_REC + NREC * NHP;   // float4 offsets inside the dynamic LDS
constexpr int LDS_BYTES = 16 * (OFF_BB + 8);   // 156 288 B; bounding boxes: NREC x 2 aux waves x {min x, min y, max x, max y}
// unit J of direction D: output slots e = 0..7 (and 8 for J = 9) are channels c = 8 J + e (c = 80 for e = 8) of that
// direction; the bwd volume runs the fwd code on the mirrored window (bwd channel c uses the offset of fwd channel 80 - c)
__host__ __device__ constexpr int cprime(int D, int J, int e) { return D ? 80 - (e < 8 ? 8 * J + e : 80) : (e < 8 ? 8 * J + e : 80); }
__host__ __device__ constexpr int qx_of(int cp) { return cp / 9 - 4; }
__host__ __device__ constexpr int qy_of(int cp) { return cp % 9 - 4; }
}  // namespace v5

// Profiling only (results are wrong): -DB2F_C5_ABLATE=bits, 1 no window DMA, 2 no unit FMAs / LDS operand reads, 4 no record stores,
// 8 no blend / halo writes, 16 no reference-tile DMA (variant 6), 32 every tile-direction takes the gather fallback (correct
// results), 64 no sampling records after the prologue (variant 6)
#ifndef B2F_C5_ABLATE
#define B2F_C5_ABLATE 0
#endif
// 1: the source window of a stage is staged in LDS by LDS-DMA where the tile-direction's taps fit it (see the header); 0: the taps
// are always gathered from memory, software-pipelined under the FMAs (measured faster so far: profiles/r03_corr_unit_kernel.txt)
#ifndef B2F_C5_WINDOW
#define B2F_C5_WINDOW 0
#endif
#ifndef B2F_C5_BATCH
#define B2F_C5_BATCH 6
#endif
// Profiling only: -DB2F_C5_TRACE=1 stamps clock64() at the phase boundaries of the first stages of block 40 (lane 0 of waves 0, 4,
// 9 and 10); the launcher prints them after the third large launch
#ifndef B2F_C5_TRACE
#define B2F_C5_TRACE 0
#endif
#if B2F_C5_TRACE
static __device__ long long c5_trace_buf[4 * 64 * 8];   // one per translation unit
#define C5_T(k_) do { if (tr_on && s < 64) c5_trace_buf[(tslot * 64 + s) * 8 + (k_)] = clock64(); } while (0)
#else
#define C5_T(k_) do {} while (0)
#endif

struct C5Tile {
    int b, y0, x0, dir;
};

// LDS-DMA of one 1-KB piece: lane i's 16 bytes at g land at LDS byte address lds + 16 i.  Not counted by the compiler's
// s_waitcnt bookkeeping: every stage ends with an explicit vmcnt(0) before its barrier.
__device__ __forceinline__ void c5_dma(const float *g, unsigned lds)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory", "m0");
}

// bounding box of a tile-direction's taps (written by the two aux waves) -> window origin, does it fit the window
// (the origin is pulled back so that the whole window lies inside the image where the image is at least that large: the DMA of
// such a window needs no clamping)
template <int NW = 2, bool WIN = (B2F_C5_WINDOW != 0)>
__device__ __forceinline__ void c5_bbox(const CorrLaunch &p, const int *bb, int &wx0, int &wy0, bool &fits)
{
    using namespace v5;
    if (!WIN) { wx0 = wy0 = 0; fits = false; return; }
    int x0 = bb[0], y0 = bb[1], x1 = bb[2], y1 = bb[3];
#pragma unroll
    for (int w = 1; w < NW; ++w) { x0 = min(x0, bb[4 * w]); y0 = min(y0, bb[4 * w + 1]); x1 = max(x1, bb[4 * w + 2]); y1 = max(y1, bb[4 * w + 3]); }
    wx0 = min(__builtin_amdgcn_readfirstlane(x0), max(p.w - WC, 0));
    wy0 = min(__builtin_amdgcn_readfirstlane(y0), max(p.h - WR, 0));
    fits = __builtin_amdgcn_readfirstlane((x1 - x0 + 1 <= WC && y1 - y0 + 1 <= WR) ? 1 : 0) != 0 && !(B2F_C5_ABLATE & 32);
}

// min / max over the 64 lanes of a wave in DPP steps (row_shr 1, 2, 4, 8, row_bcast 15, 31): the result is in lane 63
template <bool MAX>
__device__ __forceinline__ int c5_wave_reduce(int v)
{
#define C5_DPP_STEP(ctrl_, rmask_)                                                              \
    do {                                                                                        \
        const int o__ = __builtin_amdgcn_update_dpp(v, v, (ctrl_), (rmask_), 0xf, false);       \
        v = MAX ? max(v, o__) : min(v, o__);                                                    \
    } while (0)
    C5_DPP_STEP(0x111, 0xf); C5_DPP_STEP(0x112, 0xf); C5_DPP_STEP(0x114, 0xf); C5_DPP_STEP(0x118, 0xf);
    C5_DPP_STEP(0x142, 0xa); C5_DPP_STEP(0x143, 0xc);
#undef C5_DPP_STEP
    return v;
}

// flows of the three halo pixels an aux thread owns (hp = ar + 128 j)
template <int NJ = 3, int STR = 128>
__device__ __forceinline__ void c5_rec_issue(const CorrLaunch &p, const C5Tile &t, int ar, float2 &f0, float2 &f1, float2 &f2)
{
    using namespace v5;
    float2 fl[3];
    fl[2] = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int hp = ar + STR * j;
        const int hy = hp / HW, hx = hp - hy * HW;
        const int y = t.y0 - R + hy, x = t.x0 - R + hx;
        const bool in = y >= 0 && y < p.h && x >= 0 && x < p.w && hp < NHP;
        fl[j] = make_float2(0.f, 0.f);
        if (p.flow) fl[j] = *reinterpret_cast<const float2 *>(p.flow + ((size_t)t.b * p.h * p.w + (in ? (size_t)y * p.w + x : 0)) * 2);
    }
    f0 = fl[0]; f1 = fl[1]; f2 = fl[2];
}
// sampling records: clamped top-left tap (x, y: 12 bits each), "right / bottom neighbour exists" flags, valid bit, and the
// fractional weights wx, wy (getTopLeft, BilinearSamplerBHWD.cu:6-20); + this wave's bounding box of the taps
template <int NJ = 3, int STR = 128, bool WIN = (B2F_C5_WINDOW != 0)>
__device__ __forceinline__ void c5_rec_finish(const CorrLaunch &p, const C5Tile &t, int ar, float2 f0, float2 f1, float2 f2, float4 *rec, int *bbw)
{
    using namespace v5;
    const float2 fl[3] = {f0, f1, f2};
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int hp = ar + STR * j;
        const int hy = hp / HW, hx = hp - hy * HW;
        const int y = t.y0 - R + hy, x = t.x0 - R + hx;
        int packed = 0;
        float wx = 0.f, wy = 0.f;
        if (NJ * STR > NHP && hp >= NHP) continue;
        if (y >= 0 && y < p.h && x >= 0 && x < p.w) {
            const float k = t.dir == 0 ? p.k : -p.k;   // nn.MulConstant(20*(f-ref)/2^(l-2)), pwc.lua:404
            const float u = fl[j].x * k, v = fl[j].y * k;
            int xl, yt;
            bhwd_top_left(u + (float)x, p.w, xl, wx);
            bhwd_top_left(v + (float)y, p.h, yt, wy);
            const int fx = (xl + 1 <= p.w - 1) ? 1 : 0, fy = (yt + 1 <= p.h - 1) ? 1 : 0;
            packed = xl | yt << 12 | fx << 24 | fy << 25 | 1 << 26;
            if (WIN) {
                bx0 = min(bx0, xl); by0 = min(by0, yt);
                bx1 = max(bx1, xl + fx); by1 = max(by1, yt + fy);
            }
        }
        rec[hp] = make_float4(__int_as_float(packed), wx, wy, 0.f);
    }
    if (WIN) {
        bx0 = c5_wave_reduce<false>(bx0); by0 = c5_wave_reduce<false>(by0);
        bx1 = c5_wave_reduce<true>(bx1); by1 = c5_wave_reduce<true>(by1);
        if ((ar & 63) == 63) { bbw[0] = bx0; bbw[1] = by0; bbw[2] = bx1; bbw[3] = by1; }
    }
}

// taps of a stage's warped halo: thread = (halo pixel hp, 16-byte half hh), its NCC chunks, four taps each -- from the LDS
// window, or from memory (buffer loads: one scalar 128-bit resource based at the image's neighbour map, the chunk as scalar
// offset, four 32-bit lane offsets; 4 NCC loads in flight)
struct C5Samp {
    float4 w4;          // blend weights (all 0 for a halo pixel outside the image: CostVolMulti's out-of-range -> 0)
};
__device__ __forceinline__ void c5_taps(const CorrLaunch &p, const C5Tile &t, int cg, const float4 *rec, bool fits, int wx0, int wy0,
                                        const float4 *win, int hp, int hh, float4 (&tp)[4 * v5::NCC], C5Samp &sm)
{
    using namespace v5;
    const float4 r = rec[hp];
    const int packed = __float_as_int(r.x);
    const float wx = r.y, wy = r.z;
    const int xl = packed & 0xfff, yt = (packed >> 12) & 0xfff, fx = (packed >> 24) & 1, fy = (packed >> 25) & 1;
    sm.w4 = make_float4(wx * wy, (1.f - wx) * wy, wx * (1.f - wy), (1.f - wx) * (1.f - wy));
    if (!((packed >> 26) & 1)) sm.w4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (fits) {
        const int wi = ((packed >> 26) & 1) ? ((yt - wy0) * WC + (xl - wx0)) * 2 + hh : hh;
        const int dx = 2 * fx, dy = 2 * WC * fy;
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
            const float4 *wc = win + cc * (WPX * 2) + wi;
            tp[4 * cc + 0] = wc[0]; tp[4 * cc + 1] = wc[dx]; tp[4 * cc + 2] = wc[dy]; tp[4 * cc + 3] = wc[dy + dx];
        }
    } else {
        // a neighbour outside the image has weight exactly 0 (coordinates are clamped first): its address is folded onto the
        // clamped pixel instead of branching around the load
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float *>((t.dir == 0 ? p.nbr_fut : p.nbr_past) + (size_t)t.b * p.img_stride), 0, 0x7fffffff, 0x00020000);
        const int o_tl = ((yt * p.w + xl) * p.pix_stride + 4 * hh) * 4;
        const int dx = fx ? p.pix_stride * 4 : 0, dy = fy ? p.w * p.pix_stride * 4 : 0;
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
            const int so = (int)((long)(cg * NCC + cc) * p.chunk_stride * 4);
            tp[4 * cc + 0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_tl, so, 0));
            tp[4 * cc + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_tl + dx, so, 0));
            tp[4 * cc + 2] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_tl + dy, so, 0));
            tp[4 * cc + 3] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_tl + dy + dx, so, 0));
        }
    }
}
// the blend is the sampler's arithmetic ((wtl tl + wtr tr) + wbl bl) + wbr br as one mul + three fma, weights as the products
// the other kernels form -> warped halo planes
__device__ __forceinline__ void c5_blend(float4 *hdst, int hp, int hh, const float4 (&tp)[4 * v5::NCC], const C5Samp &sm)
{
    using namespace v5;
    if (B2F_C5_ABLATE & 8) return;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 WX = {sm.w4.x, sm.w4.x}, WY = {sm.w4.y, sm.w4.y}, WZ = {sm.w4.z, sm.w4.z}, WW = {sm.w4.w, sm.w4.w};
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const float4 tl = tp[4 * cc], tr = tp[4 * cc + 1], bl = tp[4 * cc + 2], br = tp[4 * cc + 3];
        // two components per instruction (v_pk_mul_f32 / v_pk_fma_f32 with the weight broadcast): the same roundings
        f32x2 lo = WX * (f32x2){tl.x, tl.y}, hi = WX * (f32x2){tl.z, tl.w};
        lo = __builtin_elementwise_fma(WY, (f32x2){tr.x, tr.y}, lo); hi = __builtin_elementwise_fma(WY, (f32x2){tr.z, tr.w}, hi);
        lo = __builtin_elementwise_fma(WZ, (f32x2){bl.x, bl.y}, lo); hi = __builtin_elementwise_fma(WZ, (f32x2){bl.z, bl.w}, hi);
        lo = __builtin_elementwise_fma(WW, (f32x2){br.x, br.y}, lo); hi = __builtin_elementwise_fma(WW, (f32x2){br.z, br.w}, hi);
        const float4 v = make_float4(lo.x, lo.y, hi.x, hi.y);
        hdst[(2 * cc + hh) * PLN + hp] = v;
    }
}

// LDS-DMA of a stage's reference tile: 8 pieces over NW waves; piece = (k4 plane, half of the tile's 128 pixels)
template <int NW = 2>
__device__ __forceinline__ void c5_ref_dma(const CorrLaunch &p, const C5Tile &t, int cg, unsigned lds_ref, int auxw, int lane)
{
    using namespace v5;
    const float *base = p.ref + (size_t)t.b * p.img_stride + (size_t)(cg * NCC) * p.chunk_stride;
#pragma unroll
    for (int j = 0; j < (2 * NK4 + NW - 1) / NW; ++j) {
        const int pc = auxw + NW * j, k4 = pc >> 1, px = 64 * (pc & 1) + lane;
        if (pc < 2 * NK4) {
            const int y = min(t.y0 + (px >> 4), p.h - 1), x = min(t.x0 + (px & 15), p.w - 1);   // ragged tiles: clamped, never stored
            c5_dma(base + (size_t)(k4 >> 1) * p.chunk_stride + (size_t)(y * p.w + x) * p.pix_stride + 4 * (k4 & 1), lds_ref + 1024u * pc);
        }
    }
}

// The tile-direction queue of a persistent block.  The macros work on the kernel's own locals: q_lin, q_tx, q_ty, q_b, q_k (newest decoded
// tile-direction), step, nmine, tiles_x, tiles_y, ncg and the five queue entries t0 .. t4.
#define C5_NEWEST(t_) do { t_.b = q_b; t_.y0 = q_ty * TH; t_.x0 = q_tx * TW; t_.dir = q_lin & 1; } while (0)
#define C5_ADVANCE()                                                              \
    do {                                                                          \
        if (q_k + 1 < nmine) {                                                    \
            ++q_k;                                                                \
            const int nl__ = q_lin + step;                                        \
            q_tx += (nl__ >> 1) - (q_lin >> 1);                                   \
            q_lin = nl__;                                                         \
            while (q_tx >= tiles_x) { q_tx -= tiles_x; ++q_ty; }                  \
            while (q_ty >= tiles_y) { q_ty -= tiles_y; ++q_b; }                   \
        }                                                                         \
    } while (0)
// tile-direction k + d (selected with scalar compares: an indexed array would live in scratch memory)
#define C5_PICK(t_, d_)                                                                                   \
    do {                                                                                                  \
        const int d__ = (d_);                                                                             \
        t_.b = d__ == 0 ? t0.b : d__ == 1 ? t1.b : d__ == 2 ? t2.b : d__ == 3 ? t3.b : t4.b;              \
        t_.y0 = d__ == 0 ? t0.y0 : d__ == 1 ? t1.y0 : d__ == 2 ? t2.y0 : d__ == 3 ? t3.y0 : t4.y0;        \
        t_.x0 = d__ == 0 ? t0.x0 : d__ == 1 ? t1.x0 : d__ == 2 ? t2.x0 : d__ == 3 ? t3.x0 : t4.x0;        \
        t_.dir = d__ == 0 ? t0.dir : d__ == 1 ? t1.dir : d__ == 2 ? t2.dir : d__ == 3 ? t3.dir : t4.dir;  \
    } while (0)
// (tile-direction offset, channel group) of the stage d stages after (tile-direction k, group cg)
#define C5_AHEAD(d_, cg_, dk_, cgo_)                               \
    do {                                                           \
        int c__ = (cg_) + (d_), dk__ = 0;                          \
        while (c__ >= ncg) { c__ -= ncg; ++dk__; }                 \
        dk_ = dk__; cgo_ = c__;                                    \
    } while (0)
#define C5_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define C5_VM_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// what the stage trace of a profiling build (B2F_C5_TRACE) prints for one kernel
struct C5TraceText { const char *label, *columns, *wave[4]; };

// persistent launch shared by the unit-form kernels: KP / KA = the instantiation for a power-of-two C / for any C, `bpc` blocks per CU
// (fewer when the launch has fewer (tile, direction) items).  Callers name <true> before <false>: the order of first use is the
// order of the kernels in the device code, which tools/device_code_diff.py compares byte for byte.
template <auto KP, auto KA>
static hipError_t launch_c5(const CorrLaunch &p, int nthr, int lds_bytes, int bpc, const C5TraceText *tr, hipStream_t s)
{
    using namespace v5;
    if (!warp_costvol_unit_supported(p)) return hipErrorInvalidValue;
    static LdsOnce once[2];
    const int slot = current_device_slot();
    const bool pow2 = (p.C & (p.C - 1)) == 0;
    if (hipError_t e = once[pow2].ensure(pow2 ? reinterpret_cast<const void *>(KP) : reinterpret_cast<const void *>(KA), lds_bytes, slot)) return e;
    const int tiles_x = (p.w + TW - 1) / TW, tiles_y = (p.h + TH - 1) / TH;
    const int ntd = 2 * tiles_x * tiles_y * p.B;
    const int cap = bpc * persistent_block_cap(slot);   // the XCD banding of the logical index wants a multiple of 8
    int grid = cap < ntd ? cap : ntd;
    if (grid >= 8) grid &= ~7;
    if (pow2) hipLaunchKernelGGL(KP, dim3((unsigned)grid), dim3((unsigned)nthr), lds_bytes, s, p, ntd, tiles_x, tiles_y);
    else hipLaunchKernelGGL(KA, dim3((unsigned)grid), dim3((unsigned)nthr), lds_bytes, s, p, ntd, tiles_x, tiles_y);
#if B2F_C5_TRACE
    static int traced = 0;
    if (tr && ntd / grid >= 50 && traced++ == 2) {
        static long long h[4 * 64 * 8];
        hipStreamSynchronize(s);
        hipMemcpyFromSymbol(h, HIP_SYMBOL(c5_trace_buf), sizeof h);
        for (int w = 0; w < 4; ++w) {
            fprintf(stderr, "%s trace %s (C %d, %d x %d): per stage, cycles: %s\n", tr->label, tr->wave[w], p.C, p.h, p.w, tr->columns);
            for (int st = 1; st < 24; ++st) {
                const long long *t = h + (w * 64 + st) * 8, *tp = h + (w * 64 + st - 1) * 8;
                fprintf(stderr, "  stage %2d  %6lld |", st, t[0] - tp[6]);
                for (int q = 1; q <= 6; ++q) fprintf(stderr, " %6lld", t[q] - t[q - 1]);
                fprintf(stderr, "   total %6lld\n", t[6] - tp[6]);
            }
        }
    }
#else
    (void)tr;
#endif
    return hipGetLastError();
}

}  // namespace b2f
