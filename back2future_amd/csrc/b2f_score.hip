// Scores against ground truth as an output stage: the evaluation of test.lua:183-261 (masked end-point error of
// criterions/L2Criterion.lua:36-38 split by the occlusion label, KITTI's Fl, the occlusion confusion matrix) on the device.
// flow_score_kernel reads every input byte once (26 B/px with everything given) and reduces the per-pixel contributions of
// b2f_flowscore.h, which the host entry (b2f_flow_score_host) shares, into one record of B2F_SCORE_WORDS integers per image: counters in
// registers, a wave reduction, the waves of a block through LDS, then at most one 64-bit atomicAdd per non-zero counter per block.
// The sums are integers, so the record does not depend on the grid or on the order of the atomics.
#include "b2f_ctx.h"
#include "b2f_flowscore.h"

using namespace b2f;

static int fail(const std::string &m) { return api_fail(m); }

namespace b2f {

namespace {

constexpr int kPx = 4;        // consecutive pixels of a plane per thread: one 16-byte load per float plane, one 4-byte load per byte plane
constexpr int kThreads = 256;
constexpr int kWave = 64;     // gfx950
constexpr int kWaves = kThreads / kWave;
constexpr int kWords = B2F_SCORE_WORDS;

// n (1..4) floats at p: one 16-byte load where the address allows (planes of odd H x W are not 16-byte aligned), scalar loads
// otherwise; v[n..] is left alone
__device__ __forceinline__ void load_f4(const float *p, int n, float *v)
{
    if (n == kPx && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) v[k] = p[k];
}

// the same for a byte plane: one 4-byte load or scalar loads
__device__ __forceinline__ void load_b4(const unsigned char *p, int n, unsigned char *v)
{
    if (n == kPx && ((uintptr_t)p & 3) == 0) {
        const uchar4 q = *reinterpret_cast<const uchar4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kPx; ++k)
        if (k < n) v[k] = p[k];
}

// Image blockIdx.y: its blocks stride over the groups of kPx pixels of the hw-pixel planes.  prob: the occlusion probabilities, or
// nullptr when the matrix is not wanted (the launcher passes it only together with gtocc).  scores[image] was zeroed on the stream.
__global__ void __launch_bounds__(kThreads) flow_score_kernel(const float *flow, const float *prob, size_t hw, double flow_scale, const float *gt,
                                                              const unsigned char *valid, const unsigned char *gtocc, unsigned long long *scores)
{
    const size_t b = blockIdx.y;
    const float *fx = flow + b * 2 * hw, *fy = fx + hw, *gx = gt + b * 2 * hw, *gy = gx + hw;
    const float *p0 = prob ? prob + b * 2 * hw : nullptr, *p1 = prob ? p0 + hw : nullptr;
    const unsigned char *va = valid ? valid + b * hw : nullptr, *lb = gtocc ? gtocc + b * hw : nullptr;
    const size_t groups = (hw + kPx - 1) / kPx;
    // a thread sees fewer than 2^28 pixels (the launcher's bound on hw): 32-bit counts, 64 bits for the Q20 sums only
    unsigned pix[4] = {0, 0, 0, 0}, outl[4] = {0, 0, 0, 0}, occ[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, nonfinite = 0;
    unsigned long long epe[4] = {0, 0, 0, 0};
    for (size_t gi = (size_t)blockIdx.x * kThreads + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * kThreads) {
        const size_t i0 = gi * kPx;
        const int n = (int)(hw - i0 < (size_t)kPx ? hw - i0 : (size_t)kPx);
        float x[kPx] = {0.f, 0.f, 0.f, 0.f}, y[kPx] = {0.f, 0.f, 0.f, 0.f}, u[kPx] = {0.f, 0.f, 0.f, 0.f}, v[kPx] = {0.f, 0.f, 0.f, 0.f};
        float q0[kPx] = {0.f, 0.f, 0.f, 0.f}, q1[kPx] = {0.f, 0.f, 0.f, 0.f};
        unsigned char ok[kPx] = {1, 1, 1, 1}, label[kPx] = {3, 3, 3, 3};
        load_f4(fx + i0, n, x);
        load_f4(fy + i0, n, y);
        load_f4(gx + i0, n, u);
        load_f4(gy + i0, n, v);
        if (va) load_b4(va + i0, n, ok);
        if (lb) load_b4(lb + i0, n, label);
        if (p0) {
            load_f4(p0 + i0, n, q0);
            load_f4(p1 + i0, n, q1);
        }
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            if (k >= n) {   // past the end of the plane: counts nowhere
                ok[k] = 0;
                label[k] = 255;
            }
            const PixelScore s = score_flow_pixel(x[k], y[k], flow_scale, u[k], v[k], ok[k], label[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hit = s.bucket == j;
                pix[j] += hit ? s.counted : 0u;
                outl[j] += hit ? s.outlier : 0u;
                epe[j] += hit ? s.q20 : 0ull;
            }
            nonfinite += s.nonfinite;
            if (p0) {
                const int cell = label[k] <= 2 ? 3 * (int)label[k] + score_occ_class(q0[k], q1[k]) : -1;
#pragma unroll
                for (int j = 0; j < 9; ++j) occ[j] += cell == j ? 1u : 0u;
            }
        }
    }
    // the record of this thread, then of its wave
    unsigned long long rec[kWords];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rec[B2F_SCORE_PIXELS + j] = pix[j];
        rec[B2F_SCORE_EPE_Q20 + j] = epe[j];
        rec[B2F_SCORE_OUTLIERS + j] = outl[j];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) rec[B2F_SCORE_OCC + j] = occ[j];
    rec[B2F_SCORE_NONFINITE] = nonfinite;
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
        if (sum) atomicAdd(scores + b * kWords + threadIdx.x, sum);
    }
}

}  // namespace

hipError_t launch_flow_score(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, const float *gt_flow,
                             const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores, hipStream_t s)
{
    const size_t hw = (size_t)H * W;
    if (n <= 0 || H <= 0 || W <= 0 || hw >= (size_t)kScoreMaxPixels || !flow || !gt_flow || !scores) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(scores, 0, (size_t)n * kWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t groups = (hw + kPx - 1) / kPx;
    // a capped grid: about eight blocks per CU over the whole call, at most 1024 per image (a full-HD image alone wraps the loop)
    const size_t cap = std::min<size_t>(1024, std::max<size_t>(8, 2048 / (size_t)n));
    const unsigned bx = (unsigned)std::min<size_t>((groups + kThreads - 1) / kThreads, cap);
    const float *prob = gt_occ ? occ_prob : nullptr;
    for (int b0 = 0; b0 < n; b0 += 65535) {   // grid.y holds 65535 images
        const int nb = std::min(n - b0, 65535);
        const size_t o = (size_t)b0 * hw;
        hipLaunchKernelGGL(flow_score_kernel, dim3(bx, (unsigned)nb), dim3(kThreads), 0, s, flow + 2 * o, prob ? prob + 2 * o : nullptr, hw, flow_scale,
                           gt_flow + 2 * o, valid ? valid + o : nullptr, gt_occ ? gt_occ + o : nullptr, scores + (size_t)b0 * kWords);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace b2f

namespace {

// what every b2f_*flow_score* entry checks before anything else
int check_flow_score(const std::string &w, const void *flow, int n, int H, int W, double flow_scale, const void *gt_flow, const void *scores)
{
    if (n <= 0 || H <= 0 || W <= 0) return fail(w + ": bad shape");
    if ((long long)H * W >= kScoreMaxPixels) return fail(w + ": images of 2^28 pixels or more are refused (the Q20 sums could overflow)");
    if (!(flow_scale > 0.0) || !std::isfinite(flow_scale)) return fail(w + ": flow_scale must be finite and > 0");
    if (!flow || !gt_flow || !scores) return fail(w + ": null argument");
    return 0;
}

}  // namespace

extern "C" {

int b2f_flow_score_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, const float *gt_flow,
                        const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores) try
{
    CHK(check_flow_score(__func__, flow, n, H, W, flow_scale, gt_flow, scores));
    flow_score_host(flow, occ_prob, n, H, W, flow_scale, gt_flow, valid, gt_occ, scores);
    return 0;
}
B2F_CATCH("b2f_flow_score_host")

int b2f_flow_score_device(b2f_ctx *c, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W, double flow_scale,
                          const float *dev_gt_flow, const unsigned char *dev_valid, const unsigned char *dev_gt_occ,
                          unsigned long long *dev_scores, void *stream) try
{
    const std::string w(__func__);
    CHK(check_flow_score(w, dev_flow, n, H, W, flow_scale, dev_gt_flow, dev_scores));
    CHK(check_device_pointers(w, c, "b2f_op_flow_score / b2f_flow_score_host", {dev_flow, dev_occ_prob, dev_gt_flow, dev_valid, dev_gt_occ, dev_scores}));
    HIPCHK(launch_flow_score(dev_flow, dev_occ_prob, n, H, W, flow_scale, dev_gt_flow, dev_valid, dev_gt_occ, dev_scores,
                             stream ? (hipStream_t)stream : c->stream));
    return 0;
}
B2F_CATCH("b2f_flow_score_device")

int b2f_op_flow_score(b2f_ctx *c, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, const float *gt_flow,
                      const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores) try
{
    CHK(check_flow_score(__func__, flow, n, H, W, flow_scale, gt_flow, scores));
    OpStage st(c, __func__);
    CHK(st.begin(true, "null context"));
    const size_t hw = (size_t)H * W, nf = (size_t)n * 2 * hw, nb = (size_t)n * hw, ns = (size_t)n * B2F_SCORE_WORDS;
    float *df, *dg, *dp = nullptr;
    unsigned char *dv = nullptr, *dl = nullptr;
    unsigned long long *ds;
    CHK(st.in(flow, nf, "flow", &df)); CHK(st.in(gt_flow, nf, "gt_flow", &dg));
    if (occ_prob) CHK(st.in(occ_prob, nf, "occ_prob", &dp));
    if (valid) CHK(st.in(valid, nb, "valid", &dv));
    if (gt_occ) CHK(st.in(gt_occ, nb, "gt_occ", &dl));
    CHK(st.out(ns, "scores", &ds));
    HIPCHK(launch_flow_score(df, dp, n, H, W, flow_scale, dg, dv, dl, ds, c->stream));
    CHK(st.finish());
    return st.get(scores, ds, ns);
}
B2F_CATCH("b2f_op_flow_score")

}  // extern "C"
