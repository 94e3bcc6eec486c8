// The unsupervised validation loss of test.lua:266-297 (the -optimize pme branch) on the device: one record of B2F_LOSS_WORDS integers
// per image and per level of the output table of model:forward.  table_loss_kernel reads the level's flows, occlusions, warped images
// and reference image once (the right and lower neighbours of the stencil through the cache), evaluates the per-pixel functions of
// b2f_tableloss.h / b2f_flowwarp.h, which the host entry (b2f_table_loss_host) shares, and reduces them like flow_warp_kernel:
// counters in registers, a wave reduction, the waves of a block through LDS, then at most one 64-bit atomicAdd per non-zero word per
// block.  The reference image of level j + 1 comes from a small pooling pass over that of level j (ref_pool_kernel), into a workspace
// of the context.
// The host half of this file is the plumbing of the whole family: the checks of the descriptor (LossSpec of b2f_ctx.h:
// which objective, which outputs), check_table, the three run paths behind table_loss_dispatch, and one body each for the *_host, *_device
// and b2f_op_* entries of all five objectives, which the one-line entries below and in b2f_tableloss_epe.hip call.
#include "b2f_ctx.h"
#include "b2f_tableloss.h"
#include "b2f_tableloss_grad_ft.h"
#include "b2f_tableloss_ssim.h"
#include "b2f_tableloss_plain.h"
#include "b2f_tableloss_grad_ssim.h"
#include "b2f_tableloss_dev.h"

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace b2f {

namespace {

constexpr int kPx = kLossPx;  // consecutive pixels of a row per thread (b2f_tableloss_dev.h: load_px)
constexpr int kThreads = kLossThreads;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kWords = B2F_LOSS_WORDS;

// Image blockIdx.y of one level: its blocks stride over the groups of kPx pixels of its rows.  loss: the record of image 0 at this
// level, image b lies `rec_stride` words further; zeroed on the stream before.
template <bool Past>
__global__ void __launch_bounds__(kThreads) table_loss_kernel(LevelPtrs lp, int h, int w, float kd, unsigned long long *loss, size_t rec_stride)
{
    const size_t b = blockIdx.y, hw = (size_t)h * w;
    constexpr int kPl = 9;   // f0 f1 p0 p1 o0 o1 R0 R1 R2 (b2f_tableloss.h: loss_pixel)
    const float *pl[kPl];
    pl[0] = lp.f + b * 2 * hw; pl[1] = pl[0] + hw;
    pl[2] = Past ? lp.p + b * 2 * hw : nullptr; pl[3] = Past ? pl[2] + hw : nullptr;
    pl[4] = lp.o + b * 2 * hw; pl[5] = pl[4] + hw;
    pl[6] = lp.ref + b * lp.ref_stride; pl[7] = pl[6] + hw; pl[8] = pl[7] + hw;
    const float *iw[2] = {lp.iw1 + b * 3 * hw, lp.iw3 + b * 3 * hw};
    const size_t gpr = ((size_t)w + kPx - 1) / kPx, groups = gpr * (size_t)h;   // groups per row, per image
    unsigned pixels = 0, nonfinite = 0, inside[2] = {0, 0}, outside[2] = {0, 0}, pnonf[2] = {0, 0};
    unsigned long long s_flow = 0, s_past = 0, s_cv = 0, s_occ = 0, s_prior = 0, ocharb[2] = {0, 0};
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const int y = (int)(gi / gpr), x0 = (int)(gi % gpr) * kPx;
        const int n = w - x0 < kPx ? w - x0 : kPx;
        const size_t i0 = (size_t)y * w + x0;
        const bool has_y = y + 1 < h, more = x0 + kPx < w;   // a row below; a pixel right of the group
        // cur[c][0..3] the group, cur[c][4] its right neighbour, low[c] the row below: every index lies in the plane (k < n, more, has_y)
        float cur[kPl][kPx + 1], low[kPl][kPx];
#pragma unroll
        for (int c = 0; c < kPl; ++c) {
#pragma unroll
            for (int k = 0; k < kPx; ++k) cur[c][k] = low[c][k] = 0.0f;
            cur[c][kPx] = 0.0f;
            if (!Past && (c == 2 || c == 3)) continue;
            load_px(pl[c] + i0, n, cur[c]);
            if (more) cur[c][kPx] = pl[c][i0 + kPx];
            if (has_y) load_px(pl[c] + i0 + w, n, low[c]);
        }
        float wv[2][3][kPx];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < kPx; ++k) wv[d][c][k] = 0.0f;
                load_px(iw[d] + (size_t)c * hw + i0, n, wv[d][c]);
            }
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const bool live = k < n;
            float v[kPl], vx[kPl], vy[kPl];
#pragma unroll
            for (int c = 0; c < kPl; ++c) {
                v[c] = cur[c][k];
                vx[c] = cur[c][k + 1];
                vy[c] = low[c][k];
            }
            const PixelLoss s = loss_pixel(v, vx, vy, x0 + k + 1 < w, has_y, Past);
            pixels += live ? 1u : 0u;
            nonfinite += live ? s.nonfinite : 0u;
            s_flow += live ? s.smooth_flow : 0ull;
            s_past += live ? s.smooth_past : 0ull;
            s_cv += live ? s.const_vel : 0ull;
            s_occ += live ? s.smooth_occ : 0ull;
            s_prior += live ? s.prior_occ : 0ull;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const bool pf = d == 0 && Past;   // OBCCriterion.lua:80-81
                // a pixel past the row's end: zero values at the group's first pixel, which is in the image; it is not counted
                const WarpTaps tp = warp_taps(pf ? v[2] : v[0], pf ? v[3] : v[1], d == 0 ? -kd : kd, live ? x0 + k : x0, y, w, h);
                const float w3[3] = {wv[d][0][k], wv[d][1][k], wv[d][2][k]}, r3[3] = {v[6], v[7], v[8]};
                const PixelPhoto ph = photo_pixel(tp, w3, r3, true, d == 0 ? v[5] : v[4]);
                inside[d] += live ? ph.inside : 0u;
                outside[d] += live ? ph.outside : 0u;
                pnonf[d] += live ? ph.nonfinite : 0u;
                ocharb[d] += live ? ph.ocharb : 0ull;
            }
        }
    }
    // the record of this thread, then of its wave
    unsigned long long rec[kWords];
    rec[B2F_LOSS_PIXELS] = pixels;
    rec[B2F_LOSS_SMOOTH_FLOW_Q30] = s_flow;
    rec[B2F_LOSS_SMOOTH_PAST_Q30] = s_past;
    rec[B2F_LOSS_CONST_VEL_Q30] = s_cv;
    rec[B2F_LOSS_SMOOTH_OCC_Q30] = s_occ;
    rec[B2F_LOSS_PRIOR_OCC_Q30] = s_prior;
    rec[B2F_LOSS_PHOTO_INSIDE] = inside[0];          rec[B2F_LOSS_PHOTO_INSIDE + 1] = inside[1];
    rec[B2F_LOSS_PHOTO_OUTSIDE] = outside[0];        rec[B2F_LOSS_PHOTO_OUTSIDE + 1] = outside[1];
    rec[B2F_LOSS_PHOTO_OCHARB_Q30] = ocharb[0];      rec[B2F_LOSS_PHOTO_OCHARB_Q30 + 1] = ocharb[1];
    rec[B2F_LOSS_PHOTO_NONFINITE] = pnonf[0];        rec[B2F_LOSS_PHOTO_NONFINITE + 1] = pnonf[1];
    rec[B2F_LOSS_NONFINITE] = nonfinite;
    rec[kWords - 1] = 0;   // reserved
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < kWords - 1; ++j) rec[j] += __shfl_down(rec[j], off, kWave);
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
        for (int wv_ = 0; wv_ < kWaves; ++wv_) sum += part[wv_][threadIdx.x];
        if (sum) atomicAdd(loss + b * rec_stride + threadIdx.x, sum);
    }
}

// R_{j+1} from R_j: the 2 x 2 mean in fp32, (((tl + tr) + bl) + br) / 4 (nn.SpatialAveragePooling(2,2,2,2), test.lua:132,269).  in:
// image 0's three planes of hi x wi, image b `in_stride` samples further; out: n x 3 x (hi / 2) x (wi / 2); one thread per output
__global__ void __launch_bounds__(kThreads) ref_pool_kernel(const float *in, size_t in_stride, int hi, int wi, size_t total, float *out)
{
    const int ho = hi / 2, wo = wi / 2;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % wo), y = (int)((i / wo) % ho), c = (int)((i / ((size_t)wo * ho)) % 3);
    const size_t b = i / ((size_t)wo * ho * 3);
    const float *q = in + b * in_stride + ((size_t)c * hi + 2 * y) * wi + 2 * x;
    out[i] = __fdiv_rn(((q[0] + q[1]) + q[wi]) + q[wi + 1], 4.0f);
}

}  // namespace

size_t table_loss_pyramid_floats(int L, int n, int H, int W)
{
    size_t t = 0;
    for (int j = 1; j < L; ++j) t += loss_level_floats(n, H >> j, W >> j);
    return t;
}

namespace {

// R_j (j >= 1) from R_{j-1}, into its place in pyr
hipError_t launch_ref_pool(const LossLevel *lv, int j, int n, float *pyr, hipStream_t s)
{
    const size_t total = (size_t)n * 3 * lv[j].h * lv[j].w;
    hipLaunchKernelGGL(ref_pool_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, lv[j - 1].lp.ref, lv[j - 1].lp.ref_stride,
                       2 * lv[j].h, 2 * lv[j].w, total, pyr + lv[j].pyr_off);
    return hipGetLastError();
}

// R_1 .. R_{L-1} alone, for a caller that wants no records
hipError_t launch_table_loss_pyramid(int L, int n, int H, int W, const float *ref, size_t ref_stride, float *pyr, hipStream_t s)
{
    LossLevel lv[kLossMaxLevels];
    if (!loss_levels(L, n, H, W, ref, ref_stride, pyr, lv)) return hipErrorInvalidValue;
    for (int j = 1; j < L; ++j) {
        const hipError_t e = launch_ref_pool(lv, j, n, pyr, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The records of test.lua:266-297: see b2f_internal.h for the arguments.  loss: n x L x words words, zeroed on s first; words:
// B2F_LOSS_WORDS, or B2F_LOSS_FT_WORDS with the words from 16 on left zero.  Lays R_1 .. R_{L-1} into pyr on the way: R_j is pooled
// behind the records of level j - 1, whose long first launch gives the host time to enqueue the rest (with all the pooling passes in
// front the stage measured 1 - 2 % slower: DESIGN.md 7.12).
hipError_t launch_table_loss(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, size_t ref_stride, float *pyr,
                             double flow_scale, unsigned long long *loss, hipStream_t s, int words)
{
    LossLevel lv[kLossMaxLevels];
    if (words < kWords || !loss || !loss_levels(table, nullptr, L, past, n, H, W, ref, ref_stride, pyr, flow_scale, lv)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(loss, 0, (size_t)n * L * words * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    for (int j = 0; j < L; ++j) {
        const LossLevel &v = lv[j];
        if (j > 0 && (e = launch_ref_pool(lv, j, n, pyr, s)) != hipSuccess) return e;
        unsigned long long *rec = loss + (size_t)j * words;
        if (past)
            hipLaunchKernelGGL(table_loss_kernel<true>, v.grid, dim3(kThreads), 0, s, v.lp, v.h, v.w, v.kd, rec, (size_t)L * words);
        else
            hipLaunchKernelGGL(table_loss_kernel<false>, v.grid, dim3(kThreads), 0, s, v.lp, v.h, v.w, v.kd, rec, (size_t)L * words);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

int ensure_dev_work(DevWork &dw, size_t bytes)
{
    if (bytes > dw.bytes) {
        if (dw.dev) {
            HIPCHK(hipDeviceSynchronize());   // an earlier call may still read it, on any stream
            HIPCHK(hipFree(dw.dev));
            dw.dev = nullptr; dw.bytes = 0;
        }
        HIPCHK(hipMalloc(&dw.dev, bytes));
        dw.bytes = bytes;
    }
    return 0;
}

}  // namespace b2f

// ---- the descriptor's checks (b2f_ctx.h: LossSpec) ----
const char *b2f::LossSpec::range_refusal() const { return ranged() ? ssim_range_refusal(range_mode, ranges) : nullptr; }

const char *b2f::LossSpec::resolve(int L)
{
    if (is_epe()) {
        if (opts) epe = *static_cast<const b2f_loss_epe_opts *>(opts);
        else (void)b2f_loss_epe_defaults(&epe);
        return loss_epe_refusal(epe, gt_flow, gt_occ, count_mode, counts, L);
    }
    if (!grad_entry) return range_refusal();
    const char *why = nullptr;
    if (obj == kLossPlain) {
        b2f_loss_grad_plain_opts t;
        if (opts) t = *static_cast<const b2f_loss_grad_plain_opts *>(opts);
        else (void)b2f_loss_grad_plain_defaults(&t);
        o = loss_grad_plain_base(t);
        ssim_alpha = t.ssim_alpha;
        plain_criterion = t.criterion;
        plain_penalty = t.penalty;
        why = loss_grad_plain_refusal(t);
    } else if (obj == kLossSsim) {
        b2f_loss_grad_ssim_opts t;
        if (opts) t = *static_cast<const b2f_loss_grad_ssim_opts *>(opts);
        else (void)b2f_loss_grad_ssim_defaults(&t);
        o = loss_grad_ssim_base(t);
        ssim_alpha = t.ssim_alpha;
        why = loss_grad_ssim_refusal(t);
    } else if (obj == kLossFt) {
        if (opts) o = *static_cast<const b2f_loss_grad_ft_opts *>(opts);
        else (void)b2f_loss_grad_ft_defaults(&o);
        why = loss_grad_ft_refusal(o);
    } else {
        b2f_loss_grad_opts t;
        if (opts) t = *static_cast<const b2f_loss_grad_opts *>(opts);
        else (void)b2f_loss_grad_defaults(&t);
        o = loss_grad_ft_from(t);
        why = loss_grad_refusal(t);
    }
    return why ? why : range_refusal();
}

int b2f::level_size(const b2f_ctx *c, int n_outs)
{
    const int own = c->past_flow ? 5 : 4, other = 9 - own;
    return (n_outs > 0 && n_outs % own == 0) ? own : (n_outs > 0 && n_outs % other == 0) ? other : 0;
}

int b2f::check_table(const std::string &w, LossSpec &d, const float *const *table, float *const *grad, const unsigned long long *loss, const float *ref,
                     int n_outs, int per, int n, int H, int W, double flow_scale, int *L)
{
    const bool epe = d.is_epe();
    if (!table || (!epe && !ref)) return fail(w + ": null argument");
    const char *why = d.outputs_refusal(loss, grad);
    if (!why) why = table_loss_refusal(n_outs, per, n, H, W, flow_scale, L);
    if (why) return fail(w + ": " + why);
    for (int i = 0; i < n_outs; ++i)
        if (!table[i]) return fail(w + ": null tensor in the table");
    // (the supervised objective says what it has to say of its options before the aliases, the others behind them)
    if (epe && (why = d.resolve(*L))) return fail(w + ": " + why);
    const void *truth[3] = {d.gt_flow, d.valid, d.gt_occ};   // null but for kLossEpe, which alone gets loss beside a gradient table here
    for (int k = 0; k < 3; ++k)
        if (epe && loss && truth[k] == (const void *)loss) return fail(w + ": loss must not alias an input");
    for (int i = 0; i < n_outs; ++i) {
        if (epe && loss && (const void *)table[i] == (const void *)loss) return fail(w + ": loss must not alias an input");
        if (!grad) continue;
        if (!grad[i]) return fail(w + ": null tensor in the gradient table");
        if (!epe && grad[i] == ref) return fail(w + ": the gradient table must not alias ref");
        if (epe && (const void *)grad[i] == (const void *)loss) return fail(w + ": the gradient table must not alias loss");
        for (int k = 0; k < 3; ++k)
            if (epe && (const void *)grad[i] == truth[k]) return fail(w + ": the gradient table must not alias the ground truth");
        for (int k = 0; k < n_outs; ++k)
            if (grad[i] == table[k] || (k != i && grad[i] == grad[k])) return fail(w + ": the gradient table must not alias the table or itself");
    }
    if (!epe && (why = d.resolve(*L))) return fail(w + ": " + why);
    return 0;
}

namespace {

// a launch on s as the row `name` of b2f_profile_read
template <class Launch>
int timed_launch(b2f_ctx *c, hipStream_t s, const char *name, Launch launch)
{
    ProfEvent pe;
    const bool timed = prof_open(c, s, name, &pe);
    const hipError_t e = launch();
    if (timed) prof_close(c, s, pe);
    HIPCHK(e);
    return 0;
}

}  // namespace

int b2f::table_loss_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, int L, bool past, int n, int H, int W, const float *dev_ref,
                        size_t ref_stride, double flow_scale, unsigned long long *dev_loss, const LossSpec &d)
{
    CHK(ensure_dev_work(c->loss_pyr, table_loss_pyramid_floats(L, n, H, W) * sizeof(float)));
    float *pyr = (float *)c->loss_pyr.dev;
    CHK(timed_launch(c, s, "table_loss", [&] {
        return launch_table_loss(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, dev_loss, s, d.words());
    }));
    if (d.ranged())
        CHK(timed_launch(c, s, "table_loss_range", [&] {
            return launch_table_loss_range(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, d.range_mode, d.ranges, dev_loss, s, d.obj == kLossPlain);
        }));
    if (d.obj == kLossPme) return 0;
    return timed_launch(c, s, d.terms_row(), [&] {
        return d.obj == kLossSsim    ? launch_table_loss_ssim_terms(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, dev_loss, s)
               : d.obj == kLossPlain ? launch_table_loss_plain_terms(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, dev_loss, s)
                                     : launch_table_loss_ft_terms(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, dev_loss, s);
    });
}

int b2f::table_loss_grad_run(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, int L, bool past, int n, int H, int W,
                             const float *dev_ref, size_t ref_stride, double flow_scale, const LossSpec &d, unsigned long long *dev_loss)
{
    const bool plain = d.obj == kLossPlain;
    GradFtCoef coef[kLossMaxLevels];
    GradCoef first[kLossMaxLevels];
    GradSsimCoef ssim[kLossMaxLevels];
    GradPlainCoef plainc[kLossMaxLevels];
    for (int j = 0; j < L; ++j) {
        loss_grad_ft_coef(d.o, j, H >> j, W >> j, &coef[j]);
        first[j] = coef[j].k;
        loss_grad_ssim_coef(d.o, d.ssim_alpha, j, H >> j, W >> j, &ssim[j]);
        if (plain) loss_grad_plain_coef(d.o, d.plain_criterion, d.plain_penalty, d.ssim_alpha, j, H >> j, W >> j, &plainc[j]);
    }
    CHK(ensure_dev_work(c->loss_pyr, table_loss_pyramid_floats(L, n, H, W) * sizeof(float)));
    if (!dev_loss) HIPCHK(launch_table_loss_pyramid(L, n, H, W, dev_ref, ref_stride, (float *)c->loss_pyr.dev, s));
    const float *pyr = (const float *)c->loss_pyr.dev;
    const unsigned long long *rec = dev_loss;
    // no records asked for: the ranges, where the criterion reads them (the SSIM + L1 term always, the plain terms with B2F_PLAIN_SSIM and a
    // pme weight), into a zeroed record buffer of the context, by the same two kernels
    if (d.ranged() && !rec && (!plain || (d.plain_criterion == B2F_PLAIN_SSIM && d.o.pme != 0.0))) {
        const size_t bytes = (size_t)n * L * d.words() * sizeof(unsigned long long);
        CHK(ensure_dev_work(c->loss_rec, bytes));
        unsigned long long *scratch = (unsigned long long *)c->loss_rec.dev;
        HIPCHK(hipMemsetAsync(scratch, 0, bytes, s));
        CHK(timed_launch(c, s, "table_loss_range", [&] {
            return launch_table_loss_range(dev_table, L, past, n, H, W, dev_ref, ref_stride, pyr, d.range_mode, d.ranges, scratch, s, plain);
        }));
        rec = scratch;
    }
    return timed_launch(c, s, d.grad_row(), [&] {
        if (d.obj == kLossPme) return launch_table_loss_grad(dev_table, dev_grad, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, first, s);
        // (ssim, plain: the flow planes by the fine-tuning kernel, the other planes by the objective's own)
        const hipError_t e = launch_table_loss_grad_ft(dev_table, dev_grad, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, coef, s, d.ranged());
        if (e != hipSuccess || !d.ranged()) return e;
        return plain ? launch_table_loss_grad_plain(dev_table, dev_grad, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, plainc, rec, s)
                     : launch_table_loss_grad_ssim(dev_table, dev_grad, L, past, n, H, W, dev_ref, ref_stride, pyr, flow_scale, ssim, rec, s);
    });
}

int b2f::table_loss_dispatch(b2f_ctx *c, hipStream_t s, const float *const *dev_table, float *const *dev_grad, unsigned long long *dev_loss, const LossSpec &d,
                             int L, bool past, int n, int H, int W, const float *dev_ref, size_t ref_stride, double flow_scale)
{
    if (d.is_epe()) return table_loss_epe_run(c, s, dev_table, dev_grad, L, past, n, H, W, flow_scale, d, dev_loss);
    if (dev_loss) CHK(table_loss_run(c, s, dev_table, L, past, n, H, W, dev_ref, ref_stride, flow_scale, dev_loss, d));
    if (dev_grad) CHK(table_loss_grad_run(c, s, dev_table, dev_grad, L, past, n, H, W, dev_ref, ref_stride, flow_scale, d, dev_loss));
    return 0;
}

int b2f::table_loss_device(const std::string &w, LossSpec d, b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                           double flow_scale, unsigned long long *dev_loss, float *const *dev_grad, void *stream)
{
    const bool epe = d.is_epe();
    const char *why;
    // (two refusals keep the place they had when the entries were written one by one: a *_grad* entry looks at its options before its
    // context, and the supervised one at the model before the table)
    if (!epe && d.grad_entry && (why = d.resolve(0))) return fail(w + ": " + why);
    if (!c) return fail(w + ": null context");
    if (epe && (why = d.model_refusal(c))) return fail(w + ": " + why);
    const int per = level_size(c, n_outs);
    if (!per) return fail(w + ": " + kTableSizeRefusal);
    int L = 0;
    CHK(check_table(w, d, dev_table, dev_grad, dev_loss, dev_ref, n_outs, per, n, H, W, flow_scale, &L));
    if (!epe && (why = d.model_refusal(c))) return fail(w + ": " + why);
    if (n > 65535) return fail(w + ": at most 65535 images per call");
    std::vector<const void *> ptrs = {dev_ref, dev_loss, d.gt_flow};
    for (int i = 0; i < n_outs; ++i) {
        ptrs.push_back(dev_table[i]);
        if (dev_grad) ptrs.push_back(dev_grad[i]);
    }
    const size_t aligned = ptrs.size();   // the byte planes may lie anywhere
    ptrs.push_back(d.valid);
    ptrs.push_back(d.gt_occ);
    CHK(check_device_pointers(w, c, d.host_entries(), ptrs.data(), ptrs.size(), aligned));
    return table_loss_dispatch(c, stream ? (hipStream_t)stream : c->stream, dev_table, dev_grad, dev_loss, d, L, per == 5, n, H, W, dev_ref, (size_t)3 * H * W,
                               flow_scale);
}

int b2f::table_loss_op(const std::string &w, LossSpec d, b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                       double flow_scale, unsigned long long *loss, float *const *grad)
{
    const bool epe = d.is_epe();
    OpStage st(c, w);
    CHK(st.begin(true, "null context"));
    const int per = level_size(c, n_outs);
    if (!per) return fail(w + ": " + kTableSizeRefusal);
    int L = 0;
    CHK(check_table(w, d, table, grad, loss, ref, n_outs, per, n, H, W, flow_scale, &L));
    const char *why = epe ? nullptr : d.model_refusal(c);   // (the supervised objective leaves the model to the device entry below)
    if (why) return fail(w + ": " + why);
    // the table and, where there is one, the gradient table, tensor by tensor; then the other inputs; then the records
    std::vector<const float *> ptrs((size_t)n_outs);
    std::vector<float *> gptrs((size_t)n_outs);
    float *df;
    for (int i = 0; i < n_outs; ++i) {
        CHK(st.in(table[i], table_floats(i, per, n, H, W), "table", &df));
        ptrs[(size_t)i] = df;
        if (grad) CHK(st.out(table_floats(i, per, n, H, W), "grad", &gptrs[(size_t)i]));
    }
    const size_t HW = (size_t)H * W, nl = (size_t)n * L * d.words();
    unsigned char *dv = nullptr, *dl = nullptr;
    unsigned long long *dloss = nullptr;
    LossSpec dd = d;
    if (epe) {
        CHK(st.in(d.gt_flow, (size_t)n * 2 * HW, "gt_flow", &df));
        if (d.valid) CHK(st.in(d.valid, (size_t)n * HW, "valid", &dv));
        if (d.gt_occ) CHK(st.in(d.gt_occ, (size_t)n * HW, "gt_occ", &dl));
        dd.gt_flow = df; dd.valid = dv; dd.gt_occ = dl;
    } else {
        CHK(st.in(ref, (size_t)n * 3 * HW, "ref", &df));
    }
    if (loss) CHK(st.out(nl, "loss", &dloss));
    // (the supervised objective's op entry has always spoken as its device entry from here on)
    CHK(table_loss_device(epe ? "b2f_table_loss_epe_device" : w, dd, c, ptrs.data(), n_outs, n, H, W, epe ? nullptr : df, flow_scale, dloss,
                          grad ? gptrs.data() : nullptr, nullptr));
    CHK(st.finish());
    if (loss) CHK(st.get(loss, dloss, nl));
    for (int i = 0; grad && i < n_outs; ++i) CHK(st.get(grad[i], gptrs[(size_t)i], table_floats(i, per, n, H, W)));
    return 0;
}

// every b2f_table_loss*_host entry: the checks, then the objective's host implementation (b2f_host.cpp)
int b2f::table_loss_host_entry(const std::string &w, LossSpec d, const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                               double flow_scale, unsigned long long *loss, float *const *grad, int rescale)
{
    int L = 0;
    const bool past = past_flow != 0;
    CHK(check_table(w, d, table, grad, loss, ref, n_outs, past ? 5 : 4, n, H, W, flow_scale, &L));
    if (d.is_epe())
        table_loss_epe_host(table, L, past, n, H, W, d.gt_flow, d.valid, d.gt_occ, flow_scale, rescale != 0, d.epe, d.count_mode, d.counts, loss, grad);
    else if (d.grad_entry && d.obj == kLossPlain)
        table_loss_grad_plain_host(table, L, past, n, H, W, ref, flow_scale, d.o, d.plain_criterion, d.plain_penalty, d.ssim_alpha, d.range_mode, d.ranges, grad);
    else if (d.grad_entry && d.obj == kLossSsim)
        table_loss_grad_ssim_host(table, L, past, n, H, W, ref, flow_scale, d.o, d.ssim_alpha, d.range_mode, d.ranges, grad);
    else if (d.grad_entry)
        table_loss_grad_ft_host(table, L, past, n, H, W, ref, flow_scale, d.o, grad);
    else if (d.obj == kLossPlain)
        table_loss_plain_host(table, L, past, n, H, W, ref, flow_scale, d.range_mode, d.ranges, loss);
    else if (d.obj == kLossSsim)
        table_loss_ssim_host(table, L, past, n, H, W, ref, flow_scale, d.range_mode, d.ranges, loss);
    else if (d.obj == kLossFt)
        table_loss_ft_host(table, L, past, n, H, W, ref, flow_scale, loss);
    else
        table_loss_host(table, L, past, n, H, W, ref, flow_scale, loss);
    return 0;
}

namespace {

// the first-order fields of the *_grad_ssim / *_grad_plain options from the defaults of b2f_loss_grad_opts
template <class Opts>
void first_order_defaults(Opts *o)
{
    b2f_loss_grad_opts t;
    (void)b2f_loss_grad_defaults(&t);
    o->smooth_flow = t.smooth_flow; o->const_vel = t.const_vel; o->pme = t.pme; o->smooth_occ = t.smooth_occ; o->prior_occ = t.prior_occ;
    for (int j = 0; j < kLossMaxLevels; ++j) o->level_weights[j] = t.level_weights[j];
    o->size_average = t.size_average;
    o->smooth_second_order = 0;
}

}  // namespace

// Every entry below builds its descriptor and calls the shared body.  *_host: on the CPU; *_device: on device pointers; b2f_op_*: on host
// pointers through the GPU.
extern "C" {

// ---- test.lua:266-297, and its gradient table of train.lua:428-468 (b2f_tableloss_grad.hip) ----
// opts.lua:61-73, test.lua:29-31
int b2f_loss_grad_defaults(b2f_loss_grad_opts *o)
{
    if (!o) return fail("b2f_loss_grad_defaults: null argument");
    o->smooth_flow = 1.0; o->const_vel = 1.0; o->pme = 1.0; o->smooth_occ = 0.1; o->prior_occ = 0.1;
    for (int j = 0; j < kLossMaxLevels; ++j) o->level_weights[j] = kLossLevelWeights[j];
    o->size_average = 0;
    return 0;
}

int b2f_table_loss_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                        unsigned long long *loss) try
{
    return table_loss_host_entry(__func__, loss_records(kLossPme), table, n_outs, n, H, W, past_flow, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_table_loss_host")

int b2f_table_loss_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                          unsigned long long *dev_loss, void *stream) try
{
    return table_loss_device(__func__, loss_records(kLossPme), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, dev_loss, nullptr, stream);
}
B2F_CATCH("b2f_table_loss_device")

int b2f_op_table_loss(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                      unsigned long long *loss) try
{
    return table_loss_op(__func__, loss_records(kLossPme), c, table, n_outs, n, H, W, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_op_table_loss")

int b2f_table_loss_grad_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                             const b2f_loss_grad_opts *opts, float *const *grad) try
{
    return table_loss_host_entry(__func__, loss_grad(opts), table, n_outs, n, H, W, past_flow, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_table_loss_grad_host")

int b2f_table_loss_grad_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                               const b2f_loss_grad_opts *opts, float *const *dev_grad, void *stream) try
{
    return table_loss_device(__func__, loss_grad(opts), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, nullptr, dev_grad, stream);
}
B2F_CATCH("b2f_table_loss_grad_device")

int b2f_op_table_loss_grad(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                           const b2f_loss_grad_opts *opts, float *const *grad) try
{
    return table_loss_op(__func__, loss_grad(opts), c, table, n_outs, n, H, W, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_op_table_loss_grad")

// ---- with the fine-tuning terms of README.md:89-102 in words 16 .. 23 (b2f_tableloss_ft.hip) and their criteria in the gradient
// (b2f_tableloss_grad_ft.hip) ----
int b2f_loss_grad_ft_defaults(b2f_loss_grad_ft_opts *o)
{
    if (!o) return fail("b2f_loss_grad_ft_defaults: null argument");
    b2f_loss_grad_opts t;
    (void)b2f_loss_grad_defaults(&t);
    *o = loss_grad_ft_from(t);
    o->smooth_second_order = 1;
    o->pme_criterion = 1;
    return 0;
}

int b2f_table_loss_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                           unsigned long long *loss) try
{
    return table_loss_host_entry(__func__, loss_records(kLossFt), table, n_outs, n, H, W, past_flow, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_table_loss_ft_host")

int b2f_table_loss_ft_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                             unsigned long long *dev_loss, void *stream) try
{
    return table_loss_device(__func__, loss_records(kLossFt), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, dev_loss, nullptr, stream);
}
B2F_CATCH("b2f_table_loss_ft_device")

int b2f_op_table_loss_ft(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                         unsigned long long *loss) try
{
    return table_loss_op(__func__, loss_records(kLossFt), c, table, n_outs, n, H, W, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_op_table_loss_ft")

int b2f_table_loss_grad_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                                const b2f_loss_grad_ft_opts *opts, float *const *grad) try
{
    return table_loss_host_entry(__func__, loss_grad(opts), table, n_outs, n, H, W, past_flow, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_table_loss_grad_ft_host")

int b2f_table_loss_grad_ft_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                                  const b2f_loss_grad_ft_opts *opts, float *const *dev_grad, void *stream) try
{
    return table_loss_device(__func__, loss_grad(opts), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, nullptr, dev_grad, stream);
}
B2F_CATCH("b2f_table_loss_grad_ft_device")

int b2f_op_table_loss_grad_ft(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                              const b2f_loss_grad_ft_opts *opts, float *const *grad) try
{
    return table_loss_op(__func__, loss_grad(opts), c, table, n_outs, n, H, W, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_op_table_loss_grad_ft")

// ---- with the SSIM + L1 sums of criterions/OSSIML1Criterion.lua:47-163 in words 16 .. 25 (b2f_tableloss_ssim.hip) and that term in the
// gradient (lines 165-302; b2f_tableloss_grad_ssim.hip) ----
int b2f_loss_grad_ssim_defaults(b2f_loss_grad_ssim_opts *o)
{
    if (!o) return fail("b2f_loss_grad_ssim_defaults: null argument");
    first_order_defaults(o);
    o->ssim_alpha = 0.85;
    return 0;
}

int b2f_table_loss_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                             unsigned long long *loss, int range_mode, const float *ranges) try
{
    return table_loss_host_entry(__func__, loss_records(kLossSsim, range_mode, ranges), table, n_outs, n, H, W, past_flow, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_table_loss_ssim_host")

int b2f_table_loss_ssim_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                               unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges) try
{
    return table_loss_device(__func__, loss_records(kLossSsim, range_mode, ranges), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, dev_loss, nullptr, stream);
}
B2F_CATCH("b2f_table_loss_ssim_device")

int b2f_op_table_loss_ssim(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                           unsigned long long *loss, int range_mode, const float *ranges) try
{
    return table_loss_op(__func__, loss_records(kLossSsim, range_mode, ranges), c, table, n_outs, n, H, W, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_op_table_loss_ssim")

int b2f_table_loss_grad_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                                  const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode, const float *ranges) try
{
    return table_loss_host_entry(__func__, loss_grad(opts, range_mode, ranges), table, n_outs, n, H, W, past_flow, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_table_loss_grad_ssim_host")

int b2f_table_loss_grad_ssim_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                                    const b2f_loss_grad_ssim_opts *opts, float *const *dev_grad, void *stream, int range_mode, const float *ranges) try
{
    return table_loss_device(__func__, loss_grad(opts, range_mode, ranges), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, nullptr, dev_grad, stream);
}
B2F_CATCH("b2f_table_loss_grad_ssim_device")

int b2f_op_table_loss_grad_ssim(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                                const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode, const float *ranges) try
{
    return table_loss_op(__func__, loss_grad(opts, range_mode, ranges), c, table, n_outs, n, H, W, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_op_table_loss_grad_ssim")

// ---- with the photometric terms without occlusion masking (criterions/MBCCriterion.lua, MSSIML1Criterion.lua): records of 40 words
// (b2f_tableloss_plain.hip) and the gradient table (b2f_tableloss_grad_plain.hip) ----
// opts.lua:61-73,85; model.lua:149-159,189-190
int b2f_loss_grad_plain_defaults(b2f_loss_grad_plain_opts *o)
{
    if (!o) return fail("b2f_loss_grad_plain_defaults: null argument");
    first_order_defaults(o);
    o->criterion = B2F_PLAIN_BCC;
    o->penalty = B2F_PLAIN_L1;
    o->ssim_alpha = 0.85;
    return 0;
}

int b2f_table_loss_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                              unsigned long long *loss, int range_mode, const float *ranges) try
{
    return table_loss_host_entry(__func__, loss_records(kLossPlain, range_mode, ranges), table, n_outs, n, H, W, past_flow, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_table_loss_plain_host")

int b2f_table_loss_plain_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                                unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges) try
{
    return table_loss_device(__func__, loss_records(kLossPlain, range_mode, ranges), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, dev_loss, nullptr, stream);
}
B2F_CATCH("b2f_table_loss_plain_device")

int b2f_op_table_loss_plain(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                            unsigned long long *loss, int range_mode, const float *ranges) try
{
    return table_loss_op(__func__, loss_records(kLossPlain, range_mode, ranges), c, table, n_outs, n, H, W, ref, flow_scale, loss, nullptr);
}
B2F_CATCH("b2f_op_table_loss_plain")

int b2f_table_loss_grad_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref, double flow_scale,
                                   const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode, const float *ranges) try
{
    return table_loss_host_entry(__func__, loss_grad(opts, range_mode, ranges), table, n_outs, n, H, W, past_flow, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_table_loss_grad_plain_host")

int b2f_table_loss_grad_plain_device(b2f_ctx *c, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref, double flow_scale,
                                     const b2f_loss_grad_plain_opts *opts, float *const *dev_grad, void *stream, int range_mode, const float *ranges) try
{
    return table_loss_device(__func__, loss_grad(opts, range_mode, ranges), c, dev_table, n_outs, n, H, W, dev_ref, flow_scale, nullptr, dev_grad, stream);
}
B2F_CATCH("b2f_table_loss_grad_plain_device")

int b2f_op_table_loss_grad_plain(b2f_ctx *c, const float *const *table, int n_outs, int n, int H, int W, const float *ref, double flow_scale,
                                 const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode, const float *ranges) try
{
    return table_loss_op(__func__, loss_grad(opts, range_mode, ranges), c, table, n_outs, n, H, W, ref, flow_scale, nullptr, grad);
}
B2F_CATCH("b2f_op_table_loss_grad_plain")

// ge, gc of the window (b2f_tableloss_ssim.h)
int b2f_loss_ssim_weights(double out[2]) try
{
    if (!out) return fail("b2f_loss_ssim_weights: null argument");
    out[0] = kSsimGe;
    out[1] = kSsimGc;
    return 0;
}
B2F_CATCH("b2f_loss_ssim_weights")

}  // extern "C"
