// Fused bilinear warp + 9x9 cost volume, "unit" form (round 3, corr_variant 5) for gfx950 (MI355X).
//
// Same arithmetic, in the same order, as the kernels of b2f_corr.hip (results are bit-identical):
//   ws[f][l] = BilinearSamplerBHWD(cs[f][l], ufs[l+1] * 20(f-2)/2^(l-1))        BilinearSamplerBHWD.cu:41-115, pwc.lua:393-409
//   fwd[c]   = 1/C * sum_k ref[y,x,k] * W3[y-qy, x-qx, k],   c = (qx+4)*9 + (qy+4)  CostVolMulti.lua:62-100
//   bwd[c]   = 1/C * sum_k ref[y,x,k] * W1[y+qy, x+qx, k]
// What is different is WHO holds the 162 sums of a pixel and HOW the neighbour map reaches the CU.
//
// The kernels of b2f_corr.hip keep 81 (or 2 x 81) accumulators per thread -- two waves per SIMD, no registers for loads in
// flight -- and gather the four bilinear taps of every halo pixel straight from memory: measured (profiles/
// r03_corr_unit_kernel.txt) a wave's 64 x 16-byte tap load costs ~45 cycles of the CU's texture-address path, 4 taps x a
// halo of 2.25 - 3 pixels per output pixel make that path, not HBM, the bound.  Here:
//
//   stage  = (tile of 8 x 16 pixels, direction, group of 16 channels);
//   window = the UNWARPED source pixels the stage's 16 x 24 halo taps fall into (bounding box of the clamped tap
//            coordinates, up to 20 x 28 pixels), brought to LDS by LDS-DMA (global_load_lds_dwordx4: no registers, 1 KB
//            contiguous per instruction -> 35 coalesced pieces instead of 96 scattered tap loads) two stages ahead;
//   blend  = warped halo of the NEXT stage from its window (4 ds_read_b128 taps per item, the sampler's arithmetic), all
//            twelve waves, LDS to LDS;
//   unit   = (stage, chunk j of 8 output channels): wave j, lane = vertical pixel pair, 16 (18 for j = 9) accumulators --
//            the two pixels of a pair share the neighbour rows (row f serves qy = -f of the upper and qy = 1 - f of the
//            lower pixel), so a unit reads ~10 neighbour float4 + 2 reference float4 from LDS per 64 - 72 FMAs;
//   block  = 12 waves (768 threads), persistent, one per CU: waves 0..9 compute one unit per stage, waves 10, 11 compute
//            the sampling records + bounding boxes of the tile-directions ahead and DMA the reference tiles.
// One LDS-only barrier per stage:  [DMA window(s+2), reference tile(s+1)] [blend halo(s+1)] [units: FMAs of s | aux: records]
// [stores of a finished tile-direction] barrier.  A tile-direction whose taps spread over more than the window holds (flow
// varying by more than ~3 pixels inside a tile) gathers its taps from memory instead, synchronously (block-uniform fallback).
// A tile's result leaves as one 32-byte chunk per pixel and unit straight from the accumulators (the record's slot order
// [fwd 0..79 | bwd 0..79 | fwd80 bwd80 u v ub vb 0 0] makes every unit one whole chunk, b2f_internal.h).
//
// This file holds variant 5 and the sixteen-wave form that ships as the default for small launches (variant 7, further down).  The
// role-specialised form (variant 6: FMA waves / gather waves, window by LDS-DMA) was measured slower at every level and lives in
// tools/experiments/csrc/b2f_corr6.hip; what it shares with the two kernels here is b2f_corr5.h.
#include "b2f_corr5.h"

namespace b2f {

template <int D, int J, int NB = B2F_C5_BATCH>
__device__ __forceinline__ void corr5_unit(const float4 *__restrict__ hb, const float4 *__restrict__ rb, float (&acc)[18])
{
    using namespace v5;
    constexpr int NE = J == 9 ? 9 : 8;
    // (column qx, row f) pairs this unit reads: every neighbour some slot's upper (f = -qy) or lower (f = 1 - qy) pixel uses
    auto used = [](int col, int f) {
        bool u = false;
        for (int e = 0; e < NE; ++e) {
            const int cp = cprime(D, J, e);
            if (qx_of(cp) == col && (-qy_of(cp) == f || 1 - qy_of(cp) == f)) u = true;
        }
        return u;
    };
#pragma unroll 1
    for (int k4 = 0; k4 < NK4; ++k4) {
        const float4 *hk = hb + k4 * PLN;
        const float4 ru = rb[k4 * (TH * TW)], rl = rb[k4 * (TH * TW) + TW];
        // the step's 10 - 11 neighbour float4 in batches of NB: a batch's LDS reads first, then its FMAs (the other two waves of
        // the SIMD cover the latency; all reads up front cost 48 registers the gather's loads in flight need)
#pragma unroll
        for (int b0 = 0; b0 < 12; b0 += NB) {
            float4 n[NB];
            {
                int i = 0;
#pragma unroll
                for (int col = -4; col <= 4; ++col)
#pragma unroll
                    for (int f = -4; f <= 5; ++f)
                        if (used(col, f)) {
                            if (i >= b0 && i < b0 + NB) n[i - b0] = hk[f * HW - col];     // fwd volume: neighbour at (y - qy, x - qx), CostVolMulti.lua:76-87
                            ++i;
                        }
            }
            __builtin_amdgcn_sched_barrier(0);
            int i = 0;
#pragma unroll
            for (int col = -4; col <= 4; ++col) {
#pragma unroll
                for (int f = -4; f <= 5; ++f) {
                    if (!used(col, f)) continue;
                    const int ii = i++;
                    if (ii < b0 || ii >= b0 + NB) continue;
                    const float4 nv = n[ii - b0];
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int cp = cprime(D, J, e);
                        if (qx_of(cp) != col) continue;
                        if (-qy_of(cp) == f) {
                            float a = acc[e];
                            a = fmaf(ru.x, nv.x, a); a = fmaf(ru.y, nv.y, a); a = fmaf(ru.z, nv.z, a); a = fmaf(ru.w, nv.w, a);
                            acc[e] = a;
                        }
                        if (1 - qy_of(cp) == f) {
                            float a = acc[9 + e];
                            a = fmaf(rl.x, nv.x, a); a = fmaf(rl.y, nv.y, a); a = fmaf(rl.z, nv.z, a); a = fmaf(rl.w, nv.w, a);
                            acc[9 + e] = a;
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// scale by 1/C (output:div(N), CostVolMulti.lua:100) and store unit j of direction d of the pixel pair.  The accumulator
// layout is the same for every unit, so direction and unit enter as (wave-uniform) run-time values: one copy of the code and
// one address computation (as template parameters the twenty chunk addresses were hoisted in front of the FMA loop)
template <bool POW2>
__device__ __forceinline__ void corr5_store(const CorrLaunch &p, const C5Tile &t, int d, int j, int pr, int lx, float (&acc)[18])
{
    using namespace v5;
    const float cf = (float)p.C, inv = 1.f / cf;
    // the addresses are formed here, after the FMA loop (hoisted in front of it they are spilled for the whole stage)
    asm volatile("" : "+v"(lx), "+v"(pr));
    const int px = t.x0 + lx;
    // wave-uniform bases + 32-bit offsets inside the image (warp_costvol_unit_supported checks that they fit)
    float *ob = p.out + (size_t)t.b * p.out_img_stride;
    float *obc = ob + (size_t)(d * 10 + j) * p.out_chunk_stride, *obl = ob + (size_t)20 * p.out_chunk_stride;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int py = t.y0 + 2 * pr + u;
        float a[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) a[e] = POW2 ? acc[9 * u + e] * inv : acc[9 * u + e] / cf;
        if (py < p.h && px < p.w && !((B2F_C5_ABLATE & 4) && a[0] != 12345.678f)) {
            const int pix = py * p.w + px;
            const unsigned off = (unsigned)(pix * p.out_pix_stride);
            float *oc = obc + off;
            *reinterpret_cast<float4 *>(oc) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4 *>(oc + 4) = make_float4(a[4], a[5], a[6], a[7]);
            if (j == 9) {   // last chunk: [fwd80, bwd80, u, v, ub, vb, 0, 0]
                float *ol = obl + off;
                if (d == 0) {
                    ol[0] = a[8];
                } else {
                    const size_t fp = ((size_t)t.b * p.h * p.w + pix) * 2;
                    float2 f = make_float2(0.f, 0.f), fb = make_float2(0.f, 0.f);
                    if (p.flow) f = *reinterpret_cast<const float2 *>(p.flow + fp);
                    if (p.flow_b) fb = *reinterpret_cast<const float2 *>(p.flow_b + fp);
                    ol[1] = a[8];
                    ol[2] = f.x; ol[3] = f.y;
                    *reinterpret_cast<float4 *>(ol + 4) = make_float4(fb.x, fb.y, 0.f, 0.f);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 18; ++e) acc[e] = 0.f;
}

// LDS-DMA of a stage's source window: 35 pieces over the 12 waves; item = 64 piece + lane -> (chunk, row, col, half), the source
// pixel clamped into the image (columns / rows past the edge re-read the edge: never used)
template <int NW = 12>
__device__ __forceinline__ void c5_win_dma(const CorrLaunch &p, const C5Tile &t, int cg, int wx0, int wy0, unsigned lds_win, int wave, int lane)
{
    using namespace v5;
    if (B2F_C5_ABLATE & 1) return;
    const float *base = (t.dir == 0 ? p.nbr_fut : p.nbr_past) + (size_t)t.b * p.img_stride + (size_t)(cg * NCC) * p.chunk_stride;
#pragma unroll
    for (int j = 0; j < (WPIECES + NW - 1) / NW; ++j) {
        const int pc = wave + NW * j;
        if (pc < WPIECES) {
            const int item = 64 * pc + lane;
            const int half = item & 1, pxi = item >> 1;
            const int cc = pxi / WPX, rr = pxi - cc * WPX;
            const int row = rr / WC, col = rr - row * WC;
            const int gy = min(wy0 + row, p.h - 1), gx = min(wx0 + col, p.w - 1);
            c5_dma(base + (size_t)cc * p.chunk_stride + (size_t)(gy * p.w + gx) * p.pix_stride + 4 * half, lds_win + 1024u * pc);
        }
    }
}

template <int D>
__device__ __forceinline__ void c5_units(int wave, const float4 *hb, const float4 *rb, float (&acc)[18])
{
    switch (wave) {
    case 0: corr5_unit<D, 0>(hb, rb, acc); break;
    case 1: corr5_unit<D, 1>(hb, rb, acc); break;
    case 2: corr5_unit<D, 2>(hb, rb, acc); break;
    case 3: corr5_unit<D, 3>(hb, rb, acc); break;
    case 4: corr5_unit<D, 4>(hb, rb, acc); break;
    case 5: corr5_unit<D, 5>(hb, rb, acc); break;
    case 6: corr5_unit<D, 6>(hb, rb, acc); break;
    case 7: corr5_unit<D, 7>(hb, rb, acc); break;
    case 8: corr5_unit<D, 8>(hb, rb, acc); break;
    default: corr5_unit<D, 9>(hb, rb, acc); break;
    }
}

// -DB2F_C5_BLOCKS=2: two blocks per CU (gather mode only: 59 KB of LDS each, 80 registers per thread)
#ifndef B2F_C5_BLOCKS
#define B2F_C5_BLOCKS 1
#endif
#if B2F_C5_BLOCKS == 2
#define C5_OCC __attribute__((amdgpu_waves_per_eu(6, 6)))
#else
#define C5_OCC
#endif
template <bool POW2>
__global__ __launch_bounds__(768) C5_OCC void warp_costvol_unit_kernel(const CorrLaunch p, const int ntd, const int tiles_x, const int tiles_y)
{
    using namespace v5;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *L = reinterpret_cast<float4 *>(smem);
    // (without the window -- B2F_C5_WINDOW 0 -- its buffers are not allocated: 59 KB, two blocks per CU fit)
    constexpr int WOFF = B2F_C5_WINDOW ? 0 : 2 * WIN_F4;
    constexpr int OFF_HALO = v5::OFF_HALO - WOFF, OFF_REF = v5::OFF_REF - WOFF, OFF_REC = v5::OFF_REC - WOFF, OFF_BB = v5::OFF_BB - WOFF;
    float4 *win = L + OFF_WIN;                                   // [2][WIN_F4]          source windows
    float4 *halo = L + OFF_HALO;                                 // [2][NK4][PLN]        warped neighbour halo of a stage
    float4 *refb = L + OFF_REF;                                  // [2][NK4][TH * TW]    reference tile of a stage
    float4 *recs = L + OFF_REC;                                  // [NREC][NHP]          sampling records of a tile-direction
    int *bbox = reinterpret_cast<int *>(L + OFF_BB);             // [NREC][2][4]
    const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>(smem));

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    const int ncg = p.C / CGC;
    const int nmine = (ntd - (int)blockIdx.x + G - 1) / G;      // tile-directions of this block: v = blockIdx.x + k G
    const int S = nmine * ncg;
    const bool aux = wave >= NUNIT;                               // waves 10, 11
    const int ar = tid - NUNIT * 64;                              // 0..127 for the aux waves
    const int ghp = tid >> 1, ghh = tid & 1;                      // blend item: halo pixel, 16-byte half of its 32-byte chunk
    const int pr = lane >> 4, lx = lane & 15;                     // unit lane: pixel-pair row, column
#if B2F_C5_TRACE
    const bool tr_on = blockIdx.x == 40 && lane == 0 && (wave == 0 || wave == 4 || wave == 9 || wave == 10) && nmine >= 50;
    const int tslot = wave == 0 ? 0 : wave == 4 ? 1 : wave == 9 ? 2 : 3;
#endif

    // ---- tile-directions k .. k + 4 of this block.  The logical index is XCD-banded like every persistent kernel here (an XCD's
    // 32 CUs walk one contiguous band of tiles, fwd / bwd of a tile on neighbouring slots: halo overlap and the shared reference
    // tile are found in that XCD's L2); consecutive tile-directions of a block are G / 8 apart, stepped without divisions.
    const int step = G >> 3;
    int q_lin, q_tx, q_ty, q_b, q_k = 0;                          // newest decoded tile-direction (index q_k)
    C5Tile t0, t1, t2, t3, t4;
    {
        q_lin = xcd_remap((int)blockIdx.x, ntd);
        const int tile = q_lin >> 1;
        q_tx = tile % tiles_x;
        q_ty = (tile / tiles_x) % tiles_y;
        q_b = tile / (tiles_x * tiles_y);
    }
    C5_NEWEST(t0); C5_ADVANCE(); C5_NEWEST(t1); C5_ADVANCE(); C5_NEWEST(t2); C5_ADVANCE(); C5_NEWEST(t3); C5_ADVANCE(); C5_NEWEST(t4);

    // ---- prologue ----
    // records of the tile-directions whose turn (three stages before their first stage) lies before stage 0; flows of the one
    // whose turn is stage 0
    float2 fa = make_float2(0.f, 0.f), fb = fa, fc = fa;          // flows in flight for the next records (aux waves)
    if (aux) {
        for (int q = 0; q < nmine && q * ncg <= 2; ++q) {
            C5Tile tt;
            C5_PICK(tt, q);
            c5_rec_issue(p, tt, ar, fa, fb, fc);
            c5_rec_finish(p, tt, ar, fa, fb, fc, recs + (q % NREC) * NHP, bbox + (q % NREC) * 8 + (wave - NUNIT) * 4);
        }
        if (3 % ncg == 0 && 3 / ncg < nmine) {
            C5Tile tt;
            C5_PICK(tt, 3 / ncg);
            c5_rec_issue(p, tt, ar, fa, fb, fc);
        }
    }
    __syncthreads();
    {   // windows of stages 0 and 1, reference tile of stage 0
        int wx0, wy0, dk, cgo;
        bool fits;
        c5_bbox(p, bbox, wx0, wy0, fits);
        if (fits) c5_win_dma(p, t0, 0, wx0, wy0, lds0 + 16u * OFF_WIN, wave, lane);
        if (1 < S) {
            C5_AHEAD(1, 0, dk, cgo);
            C5Tile tt;
            C5_PICK(tt, dk);
            c5_bbox(p, bbox + (dk % NREC) * 8, wx0, wy0, fits);
            if (fits) c5_win_dma(p, tt, cgo, wx0, wy0, lds0 + 16u * (OFF_WIN + WIN_F4), wave, lane);
        }
        if (aux) c5_ref_dma(p, t0, 0, lds0 + 16u * OFF_REF, wave - NUNIT, lane);
        C5_VM_DRAIN();
    }
    __syncthreads();
    {   // warped halo of stage 0
        int wx0, wy0;
        bool fits;
        c5_bbox(p, bbox, wx0, wy0, fits);
        float4 tp[4 * NCC];
        C5Samp sm;
        c5_taps(p, t0, 0, recs, fits, wx0, wy0, win, ghp, ghh, tp, sm);
        c5_blend(halo, ghp, ghh, tp, sm);
    }
    __syncthreads();

    // the tile-direction queue is advanced by both copies of the loop in the same way
    if (aux) {
#define C5_AUX 1
#include "b2f_corr5_loop.inc"
#undef C5_AUX
    } else {
#define C5_AUX 0
#include "b2f_corr5_loop.inc"
#undef C5_AUX
    }
}

// ---- sixteen waves (corr_variant 7): ten unit waves + six gather waves ----------------------------------------------------
// The two lessons of variants 5 and 6 put together: the FMAs want the ten 8-channel unit waves of variant 5 (a SIMD needs three
// issuing waves to retire an FMA every 1.67 cycles; one wave issues one every 5.5), and everything that waits for memory wants
// to sit in waves that do nothing else.  Block = 1 024 threads: waves 0..9 compute one unit per stage from LDS (and store a
// finished tile-direction), waves 10..15 gather the taps of the NEXT stage's warped halo straight from memory (two items = 16
// loads per thread in flight, no window), blend them into the other halo buffer, DMA the reference tile and compute the sampling
// records a stage ahead.  128 registers per thread; one LDS-only barrier per stage.

namespace v7 {
constexpr int NF = 10, NG = 6;
constexpr int NTHR = 64 * (NF + NG);            // 1 024
constexpr int GT = 64 * NG;                     // 384 gather threads
constexpr int NIT = 2 * v5::NHP / GT;           // blend items per gather thread and stage: 2
constexpr int NRJ = v5::NHP / GT;               // sampling records per gather thread and tile-direction: 1
static_assert(2 * v5::NHP % GT == 0 && v5::NHP % GT == 0 && GT % 2 == 0, "items divide over the gather threads");
constexpr int OFF_HALO = 0, OFF_REF = OFF_HALO + 2 * v5::HALO_F4, OFF_REC = OFF_REF + 2 * v5::REF_F4;
constexpr int LDS_BYTES = 16 * (OFF_REC + v5::NREC * v5::NHP);   // 84 480
}  // namespace v7

template <bool POW2>
__global__ __launch_bounds__(1024) void warp_costvol_gw_kernel(const CorrLaunch p, const int ntd, const int tiles_x, const int tiles_y)
{
    using namespace v5;
    using v7::NF;
    using v7::NG;
    using v7::GT;
    using v7::NIT;
    using v7::NRJ;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *L = reinterpret_cast<float4 *>(smem);
    float4 *halo = L + v7::OFF_HALO;
    float4 *refb = L + v7::OFF_REF;
    float4 *recs = L + v7::OFF_REC;
    const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>(smem));

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    const int ncg = p.C / CGC;
    const int nmine = (ntd - (int)blockIdx.x + G - 1) / G;
    const int S = nmine * ncg;
    const bool gth = wave >= NF;
    const int gw = wave - NF, gt = tid - NF * 64;
    const int ghp = gt >> 1, ghh = gt & 1;                        // blend items of a gather thread: halo pixels ghp + (GT / 2) i, half ghh
    const int pr = lane >> 4, lx = lane & 15;

    const int step = G >> 3;
    int q_lin, q_tx, q_ty, q_b, q_k = 0;
    C5Tile t0, t1, t2, t3, t4;
    {
        q_lin = xcd_remap((int)blockIdx.x, ntd);
        const int tile = q_lin >> 1;
        q_tx = tile % tiles_x;
        q_ty = (tile / tiles_x) % tiles_y;
        q_b = tile / (tiles_x * tiles_y);
    }
    C5_NEWEST(t0); C5_ADVANCE(); C5_NEWEST(t1); C5_ADVANCE(); C5_NEWEST(t2); C5_ADVANCE(); C5_NEWEST(t3); C5_ADVANCE(); C5_NEWEST(t4);
#define C7_TAPS(tt_, cgn_, k1_)                                                                                      \
    _Pragma("unroll") for (int i__ = 0; i__ < NIT; ++i__)                                                            \
        if (B2F_C5_ABLATE & 1) { _Pragma("unroll") for (int q__ = 0; q__ < 4 * NCC; ++q__) tp[i__][q__] = make_float4(1.f, 2.f, 3.f, 4.f); sm[i__].w4 = make_float4(.25f, .25f, .25f, .25f); } else \
        c5_taps(p, tt_, cgn_, recs + ((k1_) % NREC) * NHP, false, 0, 0, nullptr, ghp + (GT / 2) * i__, ghh, tp[i__], sm[i__])
#define C7_BLEND(hbuf_)                                                                                              \
    _Pragma("unroll") for (int i__ = 0; i__ < NIT; ++i__)                                                            \
        c5_blend(halo + (hbuf_) * HALO_F4, ghp + (GT / 2) * i__, ghh, tp[i__], sm[i__])

    // ---- prologue (gather waves): records of the first tile-directions, reference tile and warped halo of stage 0
    float2 fa = make_float2(0.f, 0.f), fb = fa, fc = fa;
    if (gth) {
        for (int q = 0; q < nmine && q * ncg <= 2; ++q) {
            C5Tile tt;
            C5_PICK(tt, q);
            c5_rec_issue<NRJ, GT>(p, tt, gt, fa, fb, fc);
            c5_rec_finish<NRJ, GT, false>(p, tt, gt, fa, fb, fc, recs + (q % NREC) * NHP, nullptr);
        }
        if (3 % ncg == 0 && 3 / ncg < nmine) {
            C5Tile tt;
            C5_PICK(tt, 3 / ncg);
            c5_rec_issue<NRJ, GT>(p, tt, gt, fa, fb, fc);
        }
        c5_ref_dma<NG>(p, t0, 0, lds0 + 16u * v7::OFF_REF, gw, lane);
    }
    __syncthreads();
    if (gth) {
        float4 tp[NIT][4 * NCC];
        C5Samp sm[NIT];
        C7_TAPS(t0, 0, 0);
        C7_BLEND(0);
        C5_VM_DRAIN();
    }
    __syncthreads();

    if (gth) {
        int s = 0;
        for (int k = 0; k < nmine; ++k) {
            for (int cg = 0; cg < ncg; ++cg, ++s) {
                const bool last_cg = cg + 1 == ncg;
                // flows of the tile-direction that stage s + 4 opens (consumed a stage later), reference tile of stage s + 1
                float2 na = fa, nb = fb, nc = fc;
                {
                    int dk, cgo;
                    C5_AHEAD(4, cg, dk, cgo);
                    if (cgo == 0 && k + dk < nmine) {
                        C5Tile tt;
                        C5_PICK(tt, dk);
                        c5_rec_issue<NRJ, GT>(p, tt, gt, na, nb, nc);
                    }
                }
                float4 tp[NIT][4 * NCC];
                C5Samp sm[NIT];
                if (s + 1 < S) {
                    C5Tile tt;
                    C5_PICK(tt, last_cg ? 1 : 0);
                    c5_ref_dma<NG>(p, tt, last_cg ? 0 : cg + 1, lds0 + 16u * (v7::OFF_REF + ((s + 1) & 1) * REF_F4), gw, lane);
                    const int k1 = last_cg ? k + 1 : k;
                    C7_TAPS(tt, last_cg ? 0 : cg + 1, k1);            // 16 loads per thread in flight under the record pass
                }
                {   // sampling records of the tile-direction that stage s + 3 opens (flows issued a stage ago)
                    int dk, cgo;
                    C5_AHEAD(3, cg, dk, cgo);
                    if (cgo == 0 && k + dk < nmine && (k + dk) * ncg > 2) {
                        C5Tile tt;
                        C5_PICK(tt, dk);
                        c5_rec_finish<NRJ, GT, false>(p, tt, gt, fa, fb, fc, recs + ((k + dk) % NREC) * NHP, nullptr);
                    }
                    fa = na; fb = nb; fc = nc;
                }
                if (s + 1 < S) C7_BLEND((s + 1) & 1);
                C5_VM_DRAIN();
                C5_LDS_BARRIER();
            }
            t0 = t1; t1 = t2; t2 = t3; t3 = t4;
            C5_ADVANCE();
            C5_NEWEST(t4);
        }
    } else {
        float acc[18];
#pragma unroll
        for (int e = 0; e < 18; ++e) acc[e] = 0.f;
        int s = 0;
        for (int k = 0; k < nmine; ++k) {
            for (int cg = 0; cg < ncg; ++cg, ++s) {
                const float4 *hb = halo + (s & 1) * HALO_F4 + (2 * pr + R) * HW + (lx + R);
                const float4 *rb = refb + (s & 1) * REF_F4 + (2 * pr) * TW + lx;
                if (!(B2F_C5_ABLATE & 2)) {
                    if (t0.dir == 0) c5_units<0>(wave, hb, rb, acc);
                    else c5_units<1>(wave, hb, rb, acc);
                }
                if (cg + 1 == ncg) corr5_store<POW2>(p, t0, t0.dir, wave, pr, lx, acc);
                C5_LDS_BARRIER();
            }
            t0 = t1; t1 = t2; t2 = t3; t3 = t4;
            C5_ADVANCE();
            C5_NEWEST(t4);
        }
    }
#undef C7_BLEND
#undef C7_TAPS
}

bool warp_costvol_unit_supported(const CorrLaunch &p)
{
    // 12-bit tap coordinates in the sampling records; 32-bit byte offsets inside an image (fallback's buffer loads)
    return p.C >= v5::CGC && p.C % v5::CGC == 0 && p.w <= 4096 && p.h <= 4096 && (double)p.img_stride * 4.0 < 2147483648.0 &&
           (double)(p.C / 8) * (double)p.chunk_stride * 4.0 + (double)p.h * p.w * p.pix_stride * 4.0 < 2147483648.0 &&
           (double)p.h * p.w * p.out_pix_stride * 4.0 < 2147483648.0;
}


hipError_t launch_warp_costvol_gw(const CorrLaunch &p, hipStream_t s)
{
    return launch_c5<&warp_costvol_gw_kernel<true>, &warp_costvol_gw_kernel<false>>(p, v7::NTHR, v7::LDS_BYTES, 1, nullptr, s);
}

hipError_t launch_warp_costvol_unit(const CorrLaunch &p, hipStream_t s)
{
    constexpr int U_LDS = v5::LDS_BYTES - (B2F_C5_WINDOW ? 0 : 16 * 2 * v5::WIN_F4);
    static const C5TraceText tr = {"c5", "top | DMA issue | blend | FMAs / records | vmcnt(0) | stores | barrier", {"wave 0", "wave 4", "wave 9", "wave 10 (aux)"}};
    return launch_c5<&warp_costvol_unit_kernel<true>, &warp_costvol_unit_kernel<false>>(p, v5::NTHR, U_LDS, B2F_C5_BLOCKS, &tr, s);
}

}  // namespace b2f
