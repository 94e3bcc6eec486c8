// Multi-GPU entry points of the C ABI (include/b2f.h, "one node, several GPUs"): what the reference gets from
// nn.DataParallelTable (util.lua:27-48: one replica per GPU, each driven by its own host thread, :34-40; batch split
// along dimension 1, :32; parameters synchronised with NCCL, train.lua:494-496) for the inference path, usable from
// the LuaJIT / C host without Python or torch:
//   * one b2f_ctx per GPU inside one process, one worker thread per GPU;
//   * the weights are loaded / generated once (GPU 0) and broadcast into every other context's flat device buffer
//     with RCCL (ncclBroadcast inside one ncclGroup, over xGMI between the GPUs of a node; the library is dlopen'ed
//     so that libb2f.so has no link-time dependency on it) or, if RCCL cannot be loaded, with hipMemcpyPeer;
//   * a batch of independent triplets is split statically and contiguously over the GPUs (sizes differ by at most
//     one, earlier GPUs take the remainder) and every worker writes straight into its slice of the caller's output
//     buffers.  No data-path collective: computeFlow keeps no cross-sample state.
#include "b2f_ctx.h"

#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <rccl/rccl.h>

using namespace b2f;

struct b2f_multi {
    std::vector<b2f_ctx *> ctx;
    std::vector<int> devices;
    int transport = 0;   // 0 = single GPU (nothing to copy), 1 = RCCL broadcast, 2 = hipMemcpyPeer
};

namespace {

struct Rccl {
    void *h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool load()
    {
        // RTLD_NOLOAD first: a host that already carries an RCCL (e.g. PyTorch's bundled copy) keeps using that one
        for (int pass = 0; pass < 2 && !h; ++pass)
            for (const char *n : {"librccl.so.1", "librccl.so"}) {
                h = dlopen(n, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
                if (h) break;
            }
        if (!h) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
        Broadcast = (decltype(Broadcast))dlsym(h, "ncclBroadcast");
        GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
        return CommInitAll && CommDestroy && GroupStart && GroupEnd && Broadcast;
    }
};

// Broadcast context 0's flat weight buffer into the others, in place on their device buffers, and rebuild their packed
// copies.  *transport: in = preferred (1 RCCL, 2 peer copy), out = used.
int broadcast_weights(b2f_multi *m, int *transport)
{
    const int n = (int)m->ctx.size();
    void *src = nullptr;
    long long count = 0;
    CHK(b2f_weights_device(m->ctx[0], &src, &count));
    std::vector<void *> dst((size_t)n, nullptr);
    for (int i = 0; i < n; ++i) {
        long long ci = 0;
        CHK(b2f_weights_device(m->ctx[i], &dst[(size_t)i], &ci));
        if (ci != count) return api_fail("b2f_init_multi: replicas disagree on the parameter count");
    }
    Rccl r;
    bool done = false;
    std::string why;
    if (*transport == 1 && r.load()) {
        // Communicators and the open group are released on every path (an early return between GroupStart and GroupEnd /
        // CommDestroy would leak all n communicators and leave RCCL's group open for the next rebroadcast): errors are
        // collected, the group is always closed, the communicators always destroyed, and ANY failure falls back to peer copies.
        std::vector<ncclComm_t> comms((size_t)n, nullptr);
        ncclResult_t rc = r.CommInitAll(comms.data(), n, m->devices.data());
        hipError_t he = hipSuccess;
        if (rc == ncclSuccess) {
            rc = r.GroupStart();
            const bool group_open = rc == ncclSuccess;
            for (int i = 0; i < n && rc == ncclSuccess && he == hipSuccess; ++i) {
                he = hipSetDevice(m->devices[(size_t)i]);
                if (he == hipSuccess)
                    rc = r.Broadcast(src, dst[(size_t)i], (size_t)count, ncclFloat, 0, comms[(size_t)i], m->ctx[(size_t)i]->stream);
            }
            if (group_open) {
                const ncclResult_t re = r.GroupEnd();
                if (rc == ncclSuccess) rc = re;
            }
            for (int i = 0; i < n; ++i) {          // drain every stream before the communicators go away, whatever happened
                hipError_t e1 = hipSetDevice(m->devices[(size_t)i]);
                if (e1 == hipSuccess) e1 = hipStreamSynchronize(m->ctx[(size_t)i]->stream);
                if (he == hipSuccess) he = e1;
            }
        }
        for (ncclComm_t c : comms)
            if (c) (void)r.CommDestroy(c);
        if (rc == ncclSuccess && he == hipSuccess) done = true;
        else why = rc != ncclSuccess ? std::string("RCCL: ") + (r.GetErrorString ? r.GetErrorString(rc) : "?") : std::string("HIP: ") + hipGetErrorString(he);
        // a HIP error here (stream sync / set device) is a faulted device, not a transport problem: no peer copies on top of it
        if (he != hipSuccess) return api_fail("b2f_init_multi: weight broadcast failed (" + why + ")");
        if (!done) fprintf(stderr, "libb2f: RCCL weight broadcast failed (%s); falling back to hipMemcpyPeer\n", why.c_str());
    } else if (*transport == 1) {
        fprintf(stderr, "libb2f: librccl.so not loadable; weight broadcast by hipMemcpyPeer\n");
    }
    if (!done) {
        *transport = 2;
        for (int i = 1; i < n; ++i) {
            if (m->devices[(size_t)i] == m->devices[0]) {
                // two replicas on one GPU (test switch B2F_MULTI_ALLOW_DUPLICATE): a peer copy onto the same device
                HIPCHK(hipSetDevice(m->devices[0]));
                HIPCHK(hipMemcpy(dst[(size_t)i], src, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice));
            } else {
                HIPCHK(hipMemcpyPeer(dst[(size_t)i], m->devices[(size_t)i], src, m->devices[0], (size_t)count * sizeof(float)));
            }
        }
    }
    for (int i = 1; i < n; ++i) CHK(b2f_commit_weights(m->ctx[(size_t)i]));
    return 0;
}

// One worker thread per GPU with a non-empty shard; `call(i, lo, hi)` runs on it.
template <class F>
int run_sharded(b2f_multi *m, int n, F call)
{
    const int g = (int)m->ctx.size();
    std::vector<int> rc((size_t)g, 0);
    std::vector<std::string> err((size_t)g);
    std::vector<std::thread> th;
    for (int i = 0; i < g; ++i) {
        int lo = 0, hi = 0;
        (void)b2f_shard_range(n, i, g, &lo, &hi);
        if (hi <= lo) continue;
        th.emplace_back([&, i, lo, hi] {
            rc[(size_t)i] = call(i, lo, hi);
            if (rc[(size_t)i]) err[(size_t)i] = api_error();   // the message is thread-local: hand it to the caller's thread
        });
    }
    for (std::thread &t : th) t.join();
    for (int i = 0; i < g; ++i)
        if (rc[(size_t)i]) return api_fail("GPU " + std::to_string(m->devices[(size_t)i]) + ": " + err[(size_t)i]);
    return 0;
}

// A host request over the replicas: replica i computes triplets [lo, hi) of the caller's n, from their inputs (a sequence: frames
// [lo, hi + 2)) into their slice of the caller's outputs.  Every shard passes the caller's n down as the request size of the kernel
// rule, so a triplet's bits do not depend on the number of GPUs.
int compute_flow_multi(b2f_multi *m, const FlowRequest &r)
{
    CHK(check_request(r));
    if (!m) return api_fail(std::string(r.who) + ": null context");
    const size_t hw = (size_t)r.H0 * r.W0, frame = 3 * hw * (r.in_kind == B2F_IN_U8 ? 1 : 4);   // bytes of an input frame
    return run_sharded(m, r.n, [&](int i, int lo, int hi) {
        auto in = [&](const void *p) { return p ? (const void *)((const char *)p + lo * frame) : nullptr; };
        FlowRequest s = r;
        s.n = hi - lo;
        s.im1 = in(r.im1); s.im2 = in(r.im2); s.im3 = in(r.im3);
        s.o = r.o.from_triplet(lo, hw);
        s.req = r.n;
        return compute_flow_host(m->ctx[(size_t)i], s);
    });
}

}  // namespace

extern "C" {

int b2f_shard_range(int n, int rank, int world, int *lo, int *hi) try
{
    if (n < 0 || world <= 0 || rank < 0 || rank >= world || !lo || !hi) return api_fail("b2f_shard_range: bad arguments");
    const int q = n / world, r = n % world;
    *lo = rank * q + std::min(rank, r);
    *hi = *lo + q + (rank < r ? 1 : 0);
    return 0;
}
B2F_CATCH("b2f_shard_range")

int b2f_init_multi(const char *name_or_path, int n_gpus, const int *devices, b2f_multi **out) try
{
    if (!out) return api_fail("b2f_init_multi: null out");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return api_fail("b2f_init_multi: no HIP device available (this library has no CPU fallback)");
    if (n_gpus == 0) n_gpus = ndev;   // all visible GPUs
    // Test switch (tests/test_gpu_parity.py: the N > 1 code path on a one-GPU box): B2F_MULTI_ALLOW_DUPLICATE=1 together with
    // B2F_MULTI_TRANSPORT=peer lets a device be listed more than once -- several replicas, worker threads and shards on one GPU
    const char *tr_env = getenv("B2F_MULTI_TRANSPORT"), *dup_env = getenv("B2F_MULTI_ALLOW_DUPLICATE");
    const bool allow_dup = dup_env && atoi(dup_env) == 1 && tr_env && !strcmp(tr_env, "peer");
    if (n_gpus < 0 || (n_gpus > ndev && !allow_dup) || n_gpus > 64) return api_fail("b2f_init_multi: n_gpus exceeds the visible devices");
    std::unique_ptr<b2f_multi> m(new b2f_multi());
    struct Guard {
        b2f_multi *m;
        ~Guard() { if (m) for (b2f_ctx *c : m->ctx) b2f_destroy(c); }
    } guard{m.get()};
    for (int i = 0; i < n_gpus; ++i) {
        const int d = devices ? devices[i] : i;
        if (d < 0 || d >= ndev) return api_fail("b2f_init_multi: bad device ordinal");
        for (int e : m->devices)
            if (e == d && !allow_dup) return api_fail("b2f_init_multi: a device is listed twice");
        m->devices.push_back(d);
    }
    // replica 0 reads the file / draws the weights; the others start from a different deterministic set of the same
    // architecture, so that only the broadcast can make them agree (b2f_multi_weights_checksum shows it)
    b2f_ctx *c0 = nullptr;
    CHK(b2f_init(name_or_path, m->devices[0], &c0));
    m->ctx.push_back(c0);
    for (int i = 1; i < n_gpus; ++i) {
        b2f_ctx *ci = nullptr;
        const std::string filler = std::string("random:") + (c0->past_flow ? "soft:" : "hard:") + std::to_string(7000 + i);
        CHK(b2f_init(filler.c_str(), m->devices[(size_t)i], &ci));
        m->ctx.push_back(ci);
    }
    const char *e = tr_env;   // "peer": skip RCCL; "selftest": run the broadcast even on one GPU
    if (n_gpus > 1 || (e && !strcmp(e, "selftest"))) {
        int transport = (e && !strcmp(e, "peer")) ? 2 : 1;
        CHK(broadcast_weights(m.get(), &transport));
        m->transport = transport;
    }
    guard.m = nullptr;
    *out = m.release();
    return 0;
}
B2F_CATCH("b2f_init_multi")

void b2f_destroy_multi(b2f_multi *m)
{
    if (!m) return;
    for (b2f_ctx *c : m->ctx) b2f_destroy(c);
    delete m;
}

int b2f_multi_info(const b2f_multi *m, int *n_gpus, int *devices, int cap, int *transport) try
{
    if (!m) return api_fail("b2f_multi_info: null context");
    if (n_gpus) *n_gpus = (int)m->ctx.size();
    if (devices)
        for (int i = 0; i < cap && i < (int)m->devices.size(); ++i) devices[i] = m->devices[(size_t)i];
    if (transport) *transport = m->transport;
    return 0;
}
B2F_CATCH("b2f_multi_info")

b2f_ctx *b2f_multi_context(b2f_multi *m, int i)
{
    return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[(size_t)i] : nullptr;
}

int b2f_multi_rebroadcast(b2f_multi *m) try
{
    if (!m) return api_fail("b2f_multi_rebroadcast: null context");
    if (m->ctx.size() < 2) return 0;
    int transport = m->transport == 2 ? 2 : 1;
    CHK(broadcast_weights(m, &transport));
    m->transport = transport;
    return 0;
}
B2F_CATCH("b2f_multi_rebroadcast")

// FNV-1a over the bits of every replica's flat weight buffer as it sits on its GPU
int b2f_multi_weights_checksum(b2f_multi *m, unsigned long long *sums, int cap) try
{
    if (!m || !sums) return api_fail("b2f_multi_weights_checksum: null argument");
    for (int i = 0; i < (int)m->ctx.size() && i < cap; ++i) {
        std::vector<float> w((size_t)m->ctx[(size_t)i]->nparams);
        CHK(b2f_get_weights(m->ctx[(size_t)i], w.data(), (long long)w.size()));
        unsigned long long h = 1469598103934665603ull;
        const unsigned char *p = (const unsigned char *)w.data();
        for (size_t k = 0; k < w.size() * sizeof(float); ++k) { h ^= p[k]; h *= 1099511628211ull; }
        sums[i] = h;
    }
    return 0;
}
B2F_CATCH("b2f_multi_weights_checksum")

int b2f_multi_compute_flow_batch(b2f_multi *m, int n, const float *im1, const float *im2, const float *im3, int H0, int W0,
                                 double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, B2F_IN_UNIT, im1, im2, im3, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_batch")

int b2f_multi_compute_flow_batch_u8(b2f_multi *m, int n, const unsigned char *im1, const unsigned char *im2, const unsigned char *im3,
                                    int H0, int W0, double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, B2F_IN_U8, im1, im2, im3, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_batch_u8")

int b2f_multi_compute_flow_sequence(b2f_multi *m, int T, const float *frames, int H0, int W0, double *flow, unsigned char *fwd_occ,
                                    unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, B2F_IN_UNIT, frames, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_sequence")

int b2f_multi_compute_flow_sequence_u8(b2f_multi *m, int T, const unsigned char *frames, int H0, int W0, double *flow,
                                       unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, B2F_IN_U8, frames, H0, W0, {flow, nullptr, nullptr, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_u8")

int b2f_multi_compute_flow_batch_f32(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                     float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0, {nullptr, flow, occ_prob, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_batch_f32")

int b2f_multi_compute_flow_sequence_f32(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, float *flow, float *occ_prob,
                                        unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0, {nullptr, flow, occ_prob, fwd_occ, bwd_occ}));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_f32")

int b2f_multi_compute_flow_batch_rgb(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                     double max_norm, int layout, unsigned char *rgb, double *max_used, float *flow, unsigned char *fwd_occ,
                                     unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                               rgb_outputs(rgb, max_used, max_norm, layout, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_batch_rgb")

int b2f_multi_compute_flow_sequence_rgb(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, double max_norm, int layout,
                                        unsigned char *rgb, double *max_used, float *flow, unsigned char *fwd_occ,
                                        unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                  rgb_outputs(rgb, max_used, max_norm, layout, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_rgb")

int b2f_multi_compute_flow_batch_score(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                       double flow_scale, const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                                       unsigned long long *scores, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                               score_outputs(flow_scale, gt_flow, valid, gt_occ, scores, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_batch_score")

int b2f_multi_compute_flow_sequence_score(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale,
                                          const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                                          unsigned long long *scores, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                  score_outputs(flow_scale, gt_flow, valid, gt_occ, scores, flow, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_score")

int b2f_multi_compute_flow_batch_warp(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                      double flow_scale, void *warped, unsigned long long *photo, float *flow, float *occ_prob,
                                      unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                               warp_outputs(flow_scale, in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_batch_warp")

int b2f_multi_compute_flow_sequence_warp(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale, void *warped,
                                         unsigned long long *photo, float *flow, float *occ_prob, unsigned char *fwd_occ,
                                         unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                  warp_outputs(flow_scale, in_kind, warped, photo, flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_warp")

int b2f_multi_compute_flow_batch_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                      float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0, past_outputs(flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_batch_past")

int b2f_multi_compute_flow_sequence_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, float *flow, float *past_flow,
                                         float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0, past_outputs(flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_past")

int b2f_multi_compute_flow_batch_warp_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3, int H0, int W0,
                                           double flow_scale, void *warped, unsigned long long *photo, float *flow, float *past_flow,
                                           float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, batch_request(__func__, n, in_kind, im1, im2, im3, H0, W0,
                                               warp_past_outputs(flow_scale, in_kind, warped, photo, flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_batch_warp_past")

int b2f_multi_compute_flow_sequence_warp_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, double flow_scale,
                                              void *warped, unsigned long long *photo, float *flow, float *past_flow, float *occ_prob,
                                              unsigned char *fwd_occ, unsigned char *bwd_occ) try
{
    return compute_flow_multi(m, sequence_request(__func__, T, in_kind, frames, H0, W0,
                                                  warp_past_outputs(flow_scale, in_kind, warped, photo, flow, past_flow, occ_prob, fwd_occ, bwd_occ)));
}
B2F_CATCH("b2f_multi_compute_flow_sequence_warp_past")

}  // extern "C"

// every b2f_multi_forward_loss* entry: the images of the request are split over the contexts, each of which runs forward_loss_host on its
// part of x, of the ground truth, of the records and of every tensor of the gradient table
static int multi_forward_loss(const std::string &w, const LossSpec &d, b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                              unsigned long long *loss, float *const *grad, int n_outs)
{
    if (!m) return api_fail(w + ": null context");
    if (!x || (d.is_epe() && !d.gt_flow) || d.outputs_refusal(loss, grad) || n <= 0 || H <= 0 || W <= 0) return api_fail(w + ": bad arguments");
    const char *why = d.sharded_refusal();
    if (why) return api_fail(w + ": " + why);
    const b2f_ctx *c0 = m->ctx[0];
    const int per = c0->past_flow ? 5 : 4, n_tab = c0->g.n_outputs();
    if (grad && n_outs != n_tab) return api_fail(w + ": n_outs must be the contexts' n_outputs");
    for (int i = 0; grad && i < n_outs; ++i)
        if (!grad[i]) return api_fail(w + ": null tensor in the gradient table");
    const size_t rec = (size_t)(n_tab / per) * d.words(), hw = (size_t)H * W;
    return run_sharded(m, n, [&](int i, int lo, int hi) {
        std::vector<float *> g((size_t)n_tab);   // the shard's part of every tensor: image lo
        for (int t = 0; grad && t < n_tab; ++t) g[(size_t)t] = grad[t] + table_floats(t, per, lo, H, W);
        return forward_loss_host(m->ctx[(size_t)i], x + (size_t)lo * 9 * hw, hi - lo, n, H, W, flow_scale, d.at_image((size_t)lo, hw),
                                 loss ? loss + (size_t)lo * rec : nullptr, grad ? g.data() : nullptr, n_outs, nullptr);
    });
}

extern "C" {

// test.lua:266-297 behind model:forward over several GPUs
int b2f_multi_forward_loss(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss) try
{
    return multi_forward_loss(__func__, loss_records(kLossPme), m, x, n, H, W, flow_scale, loss, nullptr, 0);
}
B2F_CATCH("b2f_multi_forward_loss")

// ... with the fine-tuning terms of README.md:89-102 in words 16 .. 23
int b2f_multi_forward_loss_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss) try
{
    return multi_forward_loss(__func__, loss_records(kLossFt), m, x, n, H, W, flow_scale, loss, nullptr, 0);
}
B2F_CATCH("b2f_multi_forward_loss_ft")

// ... with the SSIM + L1 sums of criterions/OSSIML1Criterion.lua:47-163 in words 16 .. 25; the batch range is refused
int b2f_multi_forward_loss_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, int range_mode,
                                const float *ranges) try
{
    return multi_forward_loss(__func__, loss_records(kLossSsim, range_mode, ranges), m, x, n, H, W, flow_scale, loss, nullptr, 0);
}
B2F_CATCH("b2f_multi_forward_loss_ssim")

// ... with the photometric sums without occlusion masking (MBCCriterion.lua, MSSIML1Criterion.lua) in words 16 .. 29; the batch range is refused
int b2f_multi_forward_loss_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss, int range_mode,
                                 const float *ranges) try
{
    return multi_forward_loss(__func__, loss_records(kLossPlain, range_mode, ranges), m, x, n, H, W, flow_scale, loss, nullptr, 0);
}
B2F_CATCH("b2f_multi_forward_loss_plain")

// the supervised objective of train.lua:296-334 behind model:forward over several GPUs; the batch's counts are refused
int b2f_multi_forward_loss_epe(b2f_multi *m, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                               const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode, const double *counts,
                               unsigned long long *loss, float *const *grad, int n_outs) try
{
    return multi_forward_loss(__func__, loss_epe(gt_flow, valid, gt_occ, opts, count_mode, counts), m, x, n, H, W, flow_scale, loss, grad, n_outs);
}
B2F_CATCH("b2f_multi_forward_loss_epe")

// the gradient table of train.lua:428-468 behind model:forward over several GPUs
int b2f_multi_forward_loss_grad(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_opts *opts,
                                unsigned long long *loss, float *const *grad, int n_outs) try
{
    return multi_forward_loss(__func__, loss_grad(opts), m, x, n, H, W, flow_scale, loss, grad, n_outs);
}
B2F_CATCH("b2f_multi_forward_loss_grad")

int b2f_multi_forward_loss_grad_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_ft_opts *opts,
                                   unsigned long long *loss, float *const *grad, int n_outs) try
{
    return multi_forward_loss(__func__, loss_grad(opts), m, x, n, H, W, flow_scale, loss, grad, n_outs);
}
B2F_CATCH("b2f_multi_forward_loss_grad_ft")

// ... with the SSIM + L1 photometric term; the batch range is refused
int b2f_multi_forward_loss_grad_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_ssim_opts *opts,
                                     unsigned long long *loss, float *const *grad, int n_outs, int range_mode, const float *ranges) try
{
    return multi_forward_loss(__func__, loss_grad(opts, range_mode, ranges), m, x, n, H, W, flow_scale, loss, grad, n_outs);
}
B2F_CATCH("b2f_multi_forward_loss_grad_ssim")

// ... with the photometric terms without occlusion masking; the batch range is refused
int b2f_multi_forward_loss_grad_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_plain_opts *opts,
                                      unsigned long long *loss, float *const *grad, int n_outs, int range_mode, const float *ranges) try
{
    return multi_forward_loss(__func__, loss_grad(opts, range_mode, ranges), m, x, n, H, W, flow_scale, loss, grad, n_outs);
}
B2F_CATCH("b2f_multi_forward_loss_grad_plain")

}  // extern "C"
