// The supervised objective (-optimize epe, opts.lua:56) on the device: the records of B2F_LOSS_EPE_WORDS integers per image and level
// and the gradient table of train.lua:296-334, with criterions/L2Criterion.lua:27-71 per pixel (b2f_tableloss_epe.h, which the host
// entry b2f_table_loss_epe_host shares).  table_loss_epe_kernel has the structure of table_loss_kernel -- a thread covers four
// consecutive pixels of a row, 16-byte loads and stores where the address allows, counters in registers, a wave reduction, the waves of
// a block through LDS, at most one 64-bit atomicAdd per non-zero word per block, the same capped grid -- without a stencil.  The ground
// truth is read in place: level j reads the full-resolution planes at (y << j, x << j) (SpatialAveragePooling(1,1,2,2),
// train.lua:282,298-299), contiguous at level 0 and at stride 2^j above it, where a level holds 4^-j of the pixels; nothing is staged.
// With -sizeAverage a gradient needs mask:sum() of L2Criterion.lua:56 before its first element: epe_count_kernel counts the valid and the
// labelled source pixels of every level first.
#include "b2f_ctx.h"
#include "b2f_tableloss_epe.h"
#include "b2f_tableloss_dev.h"

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px)
constexpr int kThreads = kLossThreads;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kWords = B2F_LOSS_EPE_WORDS;

// what a launch of one level reads and writes: image 0; image b lies 2 hw (f, o, gf, go), 2 HW (gt), HW (valid, occ), rec_stride
// (loss) or cnt_stride (cnt) elements further
struct EpeLevel {
    const float *f, *o, *gt;
    const unsigned char *valid, *occ;   // valid may be null: all valid; occ is read by the instances with Occ only
    float *gf, *go;
    unsigned long long *loss;           // null: no records
    const unsigned long long *cnt;      // N_j, N'_j as epe_count_kernel left them, or null: nf, no below
    size_t HW, rec_stride, cnt_stride;
    int h, w, j, W;
    double flow_scale, div, bf, bo, nf, no;
    int size_average;
};

// n (1..4) bytes of a row at p: one 4-byte load where the address allows, scalar loads otherwise; v[n..] is left alone
__device__ __forceinline__ void load_bytes(const unsigned char *p, int n, unsigned char *v)
{
    if (n == kPx && ((uintptr_t)p & 3) == 0) {
        const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
        v[0] = (unsigned char)(q & 255u); v[1] = (unsigned char)((q >> 8) & 255u); v[2] = (unsigned char)((q >> 16) & 255u); v[3] = (unsigned char)(q >> 24);
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) v[k] = p[k];
}

// the words of a thread summed over its block into rec[0 .. Words) of global memory: at most one atomicAdd per non-zero word
template <int Words>
__device__ __forceinline__ void block_add(unsigned long long *rec, unsigned long long *dst)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < Words; ++j) rec[j] += __shfl_down(rec[j], off, kWave);
    }
    __shared__ unsigned long long part[kWaves][Words];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < Words; ++j) part[wave][j] = rec[j];
    }
    __syncthreads();
    if (threadIdx.x < Words) {
        unsigned long long sum = 0;
        for (int wv = 0; wv < kWaves; ++wv) sum += part[wv][threadIdx.x];
        if (sum) atomicAdd(dst + threadIdx.x, sum);
    }
}

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  Records (a.loss) are zero before; every
// element of the two gradient planes (Grad) resp. of gf alone (!Occ) is written.
template <bool Grad, bool Occ>
__global__ void __launch_bounds__(kThreads) table_loss_epe_kernel(EpeLevel a)
{
    const size_t b = blockIdx.y, hw = (size_t)a.h * a.w;
    const int w = a.w, j = a.j;
    const float *f = a.f + b * 2 * hw, *o = Occ ? a.o + b * 2 * hw : nullptr, *gt = a.gt + b * 2 * a.HW;
    const unsigned char *valid = a.valid ? a.valid + b * a.HW : nullptr, *occ = Occ ? a.occ + b * a.HW : nullptr;
    double kf = 0.0, ko = 0.0;
    if (Grad) {
        kf = epe_factor(a.bf, a.size_average != 0, a.cnt ? (double)a.cnt[b * a.cnt_stride] : a.nf);
        if (Occ) ko = epe_factor(a.bo, a.size_average != 0, a.cnt ? (double)a.cnt[b * a.cnt_stride + 1] : a.no);
    }
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)a.h;   // groups per row, per image
    unsigned n_valid = 0, n_fnonf = 0, n_lab = 0, n_ononf = 0;
    unsigned long long q_flow = 0, q_occ = 0;
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const size_t s0 = ((size_t)y << j) * a.W + ((size_t)x0 << j);   // the group's first source pixel; pixel k lies k << j further
        float fv[2][kPx], gv[2][kPx], ov[2][kPx];
        unsigned char vb[kPx], lb[kPx];
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            fv[0][k] = fv[1][k] = gv[0][k] = gv[1][k] = ov[0][k] = ov[1][k] = 0.0f;
            vb[k] = 1; lb[k] = 255;
        }
        load_px(f + i0, n, fv[0]);
        load_px(f + hw + i0, n, fv[1]);
        if (Occ) {
            load_px(o + i0, n, ov[0]);
            load_px(o + hw + i0, n, ov[1]);
        }
        if (j == 0) {   // contiguous: every index is i0 + k, k < n
            load_px(gt + s0, n, gv[0]);
            load_px(gt + a.HW + s0, n, gv[1]);
            if (valid) load_bytes(valid + s0, n, vb);
            if (Occ) load_bytes(occ + s0, n, lb);
        } else {        // (y << j, (x0 + k) << j) with y < H >> j and x0 + k < W >> j lies in the plane
#pragma unroll
            for (int k = 0; k < kPx; ++k)
                if (k < n) {
                    const size_t s = s0 + ((size_t)k << j);
                    gv[0][k] = gt[s];
                    gv[1][k] = gt[a.HW + s];
                    if (valid) vb[k] = valid[s];
                    if (Occ) lb[k] = occ[s];
                }
        }
        float gfv[2][kPx], gov[2][kPx];
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const bool live = k < n;
            gfv[0][k] = gfv[1][k] = gov[0][k] = gov[1][k] = 0.0f;
            if (live && vb[k]) {
                const EpeTerm t = epe_flow_pixel(fv[0][k], fv[1][k], gv[0][k], gv[1][k], a.flow_scale, a.div, kf);
                n_valid += t.counted;
                n_fnonf += t.nonfinite;
                q_flow += t.q20;
                gfv[0][k] = (float)t.g0;
                gfv[1][k] = (float)t.g1;
            }
            if (Occ && live && epe_labelled(lb[k])) {
                const EpeTerm t = epe_occ_pixel(ov[0][k], ov[1][k], lb[k], ko);
                n_lab += t.counted;
                n_ononf += t.nonfinite;
                q_occ += t.q20;
                gov[0][k] = (float)t.g0;
                gov[1][k] = (float)t.g1;
            }
        }
        if (Grad) {
            float *gf = a.gf + b * 2 * hw;
            store_px(gf + i0, n, gfv[0]);
            store_px(gf + hw + i0, n, gfv[1]);
            if (Occ) {
                float *go = a.go + b * 2 * hw;
                store_px(go + i0, n, gov[0]);
                store_px(go + hw + i0, n, gov[1]);
            }
        }
    }
    if (!a.loss) return;   // the same for every thread of the launch
    unsigned long long rec[kWords];
    rec[B2F_LOSS_EPE_PIXELS] = 0;
    rec[B2F_LOSS_EPE_VALID] = n_valid;
    rec[B2F_LOSS_EPE_Q20] = q_flow;
    rec[B2F_LOSS_EPE_FLOW_NONFINITE] = n_fnonf;
    rec[B2F_LOSS_EPE_LABELLED] = n_lab;
    rec[B2F_LOSS_EPE_OCC_Q20] = q_occ;
    rec[B2F_LOSS_EPE_OCC_NONFINITE] = n_ononf;
    rec[kWords - 1] = 0;   // reserved
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[B2F_LOSS_EPE_PIXELS] = hw;
    block_add<kWords>(rec, a.loss + b * a.rec_stride);
}

// N_j and N'_j of image blockIdx.y: the valid (valid null: every one) and the labelled (occ null: none) source pixels of a level of
// h x w, one byte each at stride 2^j, added to cnt[b * cnt_stride + 0 | 1] (cnt_stride 0: over the batch); zero before
__global__ void __launch_bounds__(kThreads) epe_count_kernel(const unsigned char *valid, const unsigned char *occ, int h, int w, int j, int W, size_t HW,
                                                             unsigned long long *cnt, size_t cnt_stride)
{
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    unsigned long long rec[2] = {0, 0};
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (size_t)gridDim.x * kThreads) {
        const size_t y = i / (size_t)w, x = i % (size_t)w, s = b * HW + (y << j) * (size_t)W + (x << j);
        rec[0] += (!valid || valid[s]) ? 1u : 0u;
        rec[1] += (occ && epe_labelled(occ[s])) ? 1u : 0u;
    }
    block_add<2>(rec, cnt + b * cnt_stride);
}

}  // namespace

// The records and / or the gradient table of n images on s: see b2f_internal.h.
hipError_t launch_table_loss_epe(const float *const *table, float *const *grad, int L, bool past, int n, int H, int W, const float *gt_flow,
                                 const unsigned char *valid, const unsigned char *gt_occ, double flow_scale, bool rescale, const b2f_loss_epe_opts &o,
                                 int count_mode, const double *counts, unsigned long long *cnt_work, unsigned long long *loss, hipStream_t s)
{
    LossLevel lv[kLossMaxLevels];
    const bool with_occ = o.occ > 0.0;
    // the walk wants a reference image and its pyramid, which this objective has not: gt_flow stands in for both (n x 2 x H x W is not
    // n x 3 x H x W, so its stride is given as the walk's minimum); lv[j].lp.ref is not read here
    if ((!loss && !grad) || !gt_flow || (with_occ && !gt_occ) ||
        !loss_levels(table, grad, L, past, n, H, W, gt_flow, (size_t)3 * H * W, gt_flow, flow_scale, lv))
        return hipErrorInvalidValue;
    const bool counted = grad && o.size_average && count_mode != B2F_EPE_COUNT_GIVEN;
    if (counted && !cnt_work) return hipErrorInvalidValue;
    const size_t HW = (size_t)H * W, cnt_stride = count_mode == B2F_EPE_COUNT_IMAGE ? (size_t)L * 2 : 0;
    const int per = past ? 5 : 4;
    hipError_t e;
    if (loss && (e = hipMemsetAsync(loss, 0, (size_t)n * L * kWords * sizeof(unsigned long long), s)) != hipSuccess) return e;
    if (counted) {
        if ((e = hipMemsetAsync(cnt_work, 0, (count_mode == B2F_EPE_COUNT_IMAGE ? (size_t)n : 1) * L * 2 * sizeof(unsigned long long), s)) != hipSuccess) return e;
        for (int j = 0; j < L; ++j) {
            hipLaunchKernelGGL(epe_count_kernel, lv[j].grid, dim3(kThreads), 0, s, valid, with_occ ? gt_occ : nullptr, lv[j].h, lv[j].w, j, W, HW,
                               cnt_work + (size_t)j * 2, cnt_stride);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        const size_t hw = (size_t)v.h * v.w;
        // the planes of the gradient table that no kernel writes: +0.0
        for (int t = 1; grad && t < per; ++t) {
            if (t == per - 3 && with_occ) continue;
            if ((e = hipMemsetAsync(grad[(size_t)j * per + t], 0, (size_t)n * table_planes(t, per) * hw * sizeof(float), s)) != hipSuccess) return e;
        }
        EpeLevel a;
        a.f = v.lp.f; a.o = v.lp.o; a.gt = gt_flow; a.valid = valid; a.occ = gt_occ;
        a.gf = grad ? v.gp.f : nullptr; a.go = grad ? v.gp.o : nullptr;
        a.loss = loss ? loss + (size_t)j * kWords : nullptr;
        a.cnt = counted ? cnt_work + (size_t)j * 2 : nullptr;
        a.HW = HW; a.rec_stride = (size_t)L * kWords; a.cnt_stride = cnt_stride;
        a.h = v.h; a.w = v.w; a.j = j; a.W = W;
        a.flow_scale = flow_scale; a.div = rescale ? (double)(1 << j) : 1.0;
        loss_epe_base(o, j, &a.bf, &a.bo);
        a.nf = count_mode == B2F_EPE_COUNT_GIVEN && counts ? counts[2 * j] : 0.0;
        a.no = count_mode == B2F_EPE_COUNT_GIVEN && counts ? counts[2 * j + 1] : 0.0;
        a.size_average = o.size_average;
        if (grad && with_occ) hipLaunchKernelGGL((table_loss_epe_kernel<true, true>), v.grid, dim3(kThreads), 0, s, a);
        else if (grad) hipLaunchKernelGGL((table_loss_epe_kernel<true, false>), v.grid, dim3(kThreads), 0, s, a);
        else if (with_occ) hipLaunchKernelGGL((table_loss_epe_kernel<false, true>), v.grid, dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL((table_loss_epe_kernel<false, false>), v.grid, dim3(kThreads), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f

// records and / or gradient of n images on s under the profile row table_loss_epe; the counting pass, where one is needed, into c->loss_rec
int b2f::table_loss_epe_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, int L, bool past, int n, int H, int W,
                            double flow_scale, const LossSpec &d, unsigned long long *dev_loss)
{
    unsigned long long *cnt = nullptr;
    if (dev_grad && d.epe.size_average && d.count_mode != B2F_EPE_COUNT_GIVEN) {
        CHK(ensure_dev_work(c->loss_rec, (size_t)n * L * 2 * sizeof(unsigned long long)));
        cnt = (unsigned long long *)c->loss_rec.dev;
    }
    ProfEvent pe;
    const bool timed = prof_open(c, s, d.terms_row(), &pe);
    const hipError_t e = launch_table_loss_epe(dev_table, dev_grad, L, past, n, H, W, d.gt_flow, d.valid, d.gt_occ, flow_scale, c->g.rescale_flow != 0, d.epe,
                                               d.count_mode, d.counts, cnt, dev_loss, s);
    if (timed) prof_close(c, s, pe);
    HIPCHK(e);
    return 0;
}

// The entries build their descriptor and call the bodies every objective shares (b2f_tableloss.hip).
extern "C" {

// opts.lua (-epe), train.lua:56-58
int b2f_loss_epe_defaults(b2f_loss_epe_opts *o)
{
    if (!o) return fail("b2f_loss_epe_defaults: null argument");
    o->epe = 1.0; o->occ = 0.0; o->size_average = 0;
    for (int j = 0; j < kLossMaxLevels; ++j) o->level_weights[j] = kLossLevelWeights[j];
    return 0;
}

// train.lua:296-334 on the CPU
int b2f_table_loss_epe_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *gt_flow, const unsigned char *valid,
                            const unsigned char *gt_occ, double flow_scale, int rescale, const b2f_loss_epe_opts *opts, int count_mode,
                            const double *counts, unsigned long long *loss, float *const *grad) try
{
    return table_loss_host_entry(__func__, loss_epe(gt_flow, valid, gt_occ, opts, count_mode, counts), table, n_outs, n, H, W, past_flow, nullptr, flow_scale,
                                 loss, grad, rescale);
}
B2F_CATCH("b2f_table_loss_epe_host")

// train.lua:296-334 on device pointers
int b2f_table_loss_epe_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_gt_flow,
                              const unsigned char *dev_valid, const unsigned char *dev_gt_occ, double flow_scale, const b2f_loss_epe_opts *opts,
                              int count_mode, const double *counts, unsigned long long *dev_loss, float *const *dev_grad, void *stream) try
{
    return table_loss_device(__func__, loss_epe(dev_gt_flow, dev_valid, dev_gt_occ, opts, count_mode, counts), c, dev_table, n_outs, n, H, W, nullptr,
                             flow_scale, dev_loss, dev_grad, stream);
}
B2F_CATCH("b2f_table_loss_epe_device")

// train.lua:296-334 on host pointers through the GPU: every buffer in the guarded staging scope
int b2f_op_table_loss_epe(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                          const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode, const double *counts,
                          unsigned long long *loss, float *const *grad) try
{
    return table_loss_op(__func__, loss_epe(gt_flow, valid, gt_occ, opts, count_mode, counts), c, table, n_outs, n, H, W, nullptr, flow_scale, loss, grad);
}
B2F_CATCH("b2f_op_table_loss_epe")

}  // extern "C"
