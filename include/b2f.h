/*
 * b2f.h -- C ABI of libb2f.so: the MI355X-native (gfx950) drop-in for the
 * back2future `init()` -> `computeFlow(im1, im2, im3)` hot path.
 *
 * The reference has no C ABI for this path: its native boundary is the Torch7
 * Lua-C extension protocol (luaL_Reg tables on the tensor metatable,
 * /root/reference/extras/stnbhwd/BilinearSamplerBHWD.cu:423-435, init.cu:11-18)
 * and, above it, the Lua function pair exported by back2future.lua:45,97-130.
 * Each entry point below cites the reference interface it replaces.  The
 * LuaJIT-ffi / ctypes bindings that call this header are shown in
 * INTEGRATION.md.
 *
 * Conventions: every call returns 0 on success, non-zero on error with a
 * thread-local message readable through b2f_last_error() (the Lua shim turns
 * it into error(msg), mirroring THError at BilinearSamplerBHWD.cu:151-156).
 * Plain pointers and sizes only; the caller owns every buffer it passes in;
 * the library owns device memory inside the opaque context.  A context is
 * bound to one GPU; several GPUs of a node are driven either by one process per GPU
 * (one context per rank, the host broadcasts the flat weight buffer over RCCL, see
 * b2f_weights_device) or by one b2f_multi inside one process (b2f_init_multi below).
 * "host" pointers are CPU memory, "dev" pointers are HIP device memory on the
 * context's GPU.  `stream` is a hipStream_t passed as void* (NULL = the
 * context's own stream).
 */
#ifndef B2F_H
#define B2F_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define B2F_API __attribute__((visibility("default")))
#else
#define B2F_API
#endif

typedef struct b2f_ctx b2f_ctx;

/* Error text of the last failing call on this thread ("" if none). */
B2F_API const char *b2f_last_error(void);

/* Library/ABI version (major*1000 + minor). */
B2F_API int b2f_version(void);

/* ---- life cycle: replaces back2future.init(opt) (back2future.lua:97-129) ----
 * name_or_path:
 *   "Ours-Hard" | "Ours-Soft-ft-KITTI" | "Ours-Soft-ft-Sintel"
 *        -> models/RoamingImages_H.t7 | _H_KITTI_S.t7 | _H_Sintel_S.t7 relative to
 *           the current directory, exactly as back2future.lua:100-110 (error if absent)
 *   a path ending in ".t7"    -> Torch7 serialized nn.gModule / DataParallelTable
 *   a path ending in ".b2fw"  -> flat fp32 blob in this repo's canonical order
 *   "random:hard[:seed[:gain]]" | "random:soft[:seed[:gain]]"
 *        -> the pwc.lua architecture with deterministic random weights
 *           (nn.SpatialConvolution:reset() distribution), for synthetic benchmarks.
 * device: HIP device ordinal.                                                    */
B2F_API int b2f_init(const char *name_or_path, int device, b2f_ctx **out);
/* Same with the graph shape of createModelMulti(opt) (models/pwc.lua:88-121) given explicitly, for models other
 * than the shipped ones: graph_opts = "win=5,levels=4" (createModelMulti(nil), pwc.lua:88), or any subset of
 * win (pwc_ws), levels, skip (pwc_skip, >= 0), two_frame, sum_cvs (pwc_sum_cvs), residual, occ_input,
 * rescale_flow, flownet_factor, siamese (pwc_siamese); NULL / "" = the shipped graph (opts.lua:83-98) -- or, for a ".t7" file, whatever
 * shape the file holds: win is read from its nn.CostVolMulti nodes (CostVolMulti.lua:26-37), levels and skip from the
 * convUnits / decoders in its node list (pwc.lua:136,237), the other options stay at their defaults; with graph_opts
 * given the file must be that graph.  frames = 3 is fixed; a pwc_siamese = 0 model (no convUnits: decoders of every
 * level have the same shapes) is not read from .t7, only from flat weights.  Weights: "random:hard|soft[:seed[:gain]]", a ".t7" file or a .b2fw blob in the canonical order of that graph
 * (feature units l = 2..levels -- from l = 1 with skip = 0, none with siamese = 0 --, then l = levels..skip+1 {occ, flow,
 * [past-flow] decoder}).  Non-shipped shapes run
 * on a generic, untuned executor (every Lua node its own kernels); H and W of b2f_forward must then be multiples
 * of 2^(levels-1), computeFlow keeps the reference's /64 rounding.                                            */
B2F_API int b2f_init_ex(const char *name_or_path, int device, const char *graph_opts, b2f_ctx **out);
B2F_API void b2f_destroy(b2f_ctx *ctx);

/* levels (7), cost-volume window (9), past_flow (0 Hard / 1 Soft), number of
 * tensors in the model:forward output table ((levels - skip) x 4 | 5: 20 / 25 for the shipped
 * models, pwc.lua:459-489), #params. */
B2F_API int b2f_info(const b2f_ctx *ctx, int *levels, int *win, int *past_flow, int *n_outputs,
             long long *n_params);

/* ---- weights (the .t7 payload of back2future.lua:113) ----
 * Canonical flat order: feature units l=2..7 {conv1.w,b,conv2.w,b};
 * then l=7..3 {occ decoder, flow decoder, [past-flow decoder]} x 6 x {w,b};
 * every w is Co x Ci x 3 x 3 as in nn.SpatialConvolution.                        */
B2F_API long long b2f_param_count(int past_flow);
/* Host-only, no GPU needed: fills out[n] with the deterministic random init. */
B2F_API int b2f_random_weights(unsigned long long seed, int past_flow, float gain, float *out,
                       long long n);
B2F_API int b2f_set_weights(b2f_ctx *ctx, const float *host_flat, long long n);
B2F_API int b2f_get_weights(b2f_ctx *ctx, float *host_flat, long long n);
/* Device address of the flat canonical buffer, so that the host can broadcast it in
 * place with RCCL (torch.distributed.broadcast) -- this replaces the NCCL parameter
 * sync of nn.DataParallelTable (util.lua:27-48, train.lua:494-496).  Call
 * b2f_commit_weights afterwards to rebuild the kernel-side packed copies.          */
B2F_API int b2f_weights_device(b2f_ctx *ctx, void **dev_ptr, long long *n);
B2F_API int b2f_commit_weights(b2f_ctx *ctx);
/* Host-only .t7 reader (replaces torch.load + nngraph walk): fills out[n] in canonical
 * order and sets *past_flow.  No GPU needed.                                       */
B2F_API int b2f_load_t7(const char *path, float *out, long long cap, long long *n, int *past_flow);
/* The same for any graph shape (torch.load of a model built by createModelMulti(opt), pwc.lua:88-121): graph_opts NULL / "" =
 * read win / levels / skip from the file, else the file must be that graph; opts_out (optional, opts_cap bytes) receives the
 * graph as an option string ("win=5,levels=4,skip=2,...,past_flow=1"), out[n] the weights in that graph's canonical order. */
B2F_API int b2f_load_t7_ex(const char *path, const char *graph_opts, float *out, long long cap, long long *n, char *opts_out,
                   int opts_cap);

/* ---- the hot path, host boundary: computeFlow (back2future.lua:47-95) ----
 * im1..im3: 3 x H0 x W0 planar RGB floats in [0,1] (what image.load returns).
 * flow: 2 x H0 x W0 doubles (raw network flow, channel 0 = x, rescaled to H0 x W0
 * exactly as :80-84);  fwd_occ / bwd_occ: H0 x W0 bytes (0/1), thresholds of
 * est[3][2] / est[3][1] at 0.6666 (:87-91).                                        */
B2F_API int b2f_compute_flow(b2f_ctx *ctx, const float *im1, const float *im2, const float *im3,
                     int H0, int W0, double *flow, unsigned char *fwd_occ,
                     unsigned char *bwd_occ);
/* Same on n independent triplets (host buffers, n x 3 x H0 x W0 each frame set; outputs
 * n x 2 x H0 x W0 and n x H0 x W0).  The library overlaps uploads, kernels and downloads
 * of consecutive sub-batches; planes whose values are all k/255 cross the link as bytes
 * (rebuilt bit for bit on the device), the flow as fp32 widened on the host.          */
B2F_API int b2f_compute_flow_batch(b2f_ctx *ctx, int n, const float *im1, const float *im2,
                           const float *im3, int H0, int W0, double *flow,
                           unsigned char *fwd_occ, unsigned char *bwd_occ);
/* Same for frames that are still 8-bit (n x 3 x H0 x W0 bytes, planar RGB): the value of a
 * sample is byte / 255, the float image.load() [torch/image] makes of it, so the results are
 * those of b2f_compute_flow_batch on the converted floats, bit for bit, at a quarter of the
 * upload ("n x 9 x H x W f32 or ... u8").                                     */
B2F_API int b2f_compute_flow_batch_u8(b2f_ctx *ctx, int n, const unsigned char *im1,
                              const unsigned char *im2, const unsigned char *im3, int H0, int W0,
                              double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);

/* ---- one node, several GPUs: replaces nn.DataParallelTable (util.lua:27-48) for this path ----
 * One context per GPU inside the calling process, one library worker thread per GPU (the
 * reference's replicas each run on their own thread, util.lua:34-40).  b2f_init_multi loads /
 * generates the weights once (first device) and broadcasts them into the other replicas' device
 * buffers with RCCL (ncclBroadcast, xGMI inside a node; dlopen'ed) or hipMemcpyPeer when RCCL is
 * not loadable -- the NCCL parameter sync of train.lua:494-496.  devices: n_gpus ordinals or NULL
 * (0 .. n_gpus-1); n_gpus = 0 takes every visible GPU.  The batch entry points split the n triplets
 * statically and contiguously over the GPUs (b2f_shard_range: the dim-1 split of util.lua:32;
 * sizes differ by at most one) and every GPU writes straight into its slice of the caller's
 * buffers; same arguments and results as b2f_compute_flow_batch[_u8].                          */
typedef struct b2f_multi b2f_multi;
B2F_API int b2f_init_multi(const char *name_or_path, int n_gpus, const int *devices, b2f_multi **out);
B2F_API void b2f_destroy_multi(b2f_multi *m);
/* transport: 0 one GPU, 1 RCCL broadcast, 2 hipMemcpyPeer */
B2F_API int b2f_multi_info(const b2f_multi *m, int *n_gpus, int *devices, int cap, int *transport);
/* the i-th replica (for b2f_info / b2f_set_option / b2f_set_weights on replica 0 followed by
 * b2f_multi_rebroadcast); NULL if out of range.  Owned by m.                                    */
B2F_API b2f_ctx *b2f_multi_context(b2f_multi *m, int i);
B2F_API int b2f_multi_rebroadcast(b2f_multi *m);
/* FNV-1a of every replica's weight buffer as it sits on its GPU: equal after a broadcast        */
B2F_API int b2f_multi_weights_checksum(b2f_multi *m, unsigned long long *sums, int cap);
/* host-only: [lo, hi) of `rank` when n items are split over `world` GPUs                         */
B2F_API int b2f_shard_range(int n, int rank, int world, int *lo, int *hi);
B2F_API int b2f_multi_compute_flow_batch(b2f_multi *m, int n, const float *im1, const float *im2,
                                 const float *im3, int H0, int W0, double *flow,
                                 unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_batch_u8(b2f_multi *m, int n, const unsigned char *im1,
                                    const unsigned char *im2, const unsigned char *im3, int H0, int W0,
                                    double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);

/* ---- the hot path, device boundary: model:forward(imgs) (back2future.lua:74) ----
 * dev_in: B x 9 x H x W planar fp32 on the GPU (the tensor `imgs` of :73), H and W
 * multiples of 64.  in_kind: B2F_IN_NORMALIZED = already colour-normalized (what the
 * reference feeds the model), B2F_IN_UNIT = raw [0,1] values, normalized on device.
 * Outputs (any may be NULL), all planar fp32 on the GPU:
 *   dev_flow  B x 2 x H x W   est[1] = skip_ufs[3]
 *   dev_occ   B x 2 x H x W   skip_occs[3] (softmax probabilities)
 *   dev_est3  B x C3 x H x W  est[3] as computeFlow reads it: C3 = 2 (Soft: the
 *                             occlusion map) or 3 (Hard: warped image 1)
 * Every device pointer must be 16-byte aligned (vector loads / stores; hipMalloc and torch
 * allocations are, a view at an odd storage offset is not): a misaligned one is rejected.
 * The call is asynchronous on `stream`; the context's own stream (NULL) is a blocking stream
 * (ordered with the legacy default stream, not with other non-blocking streams); results are
 * awaited with b2f_synchronize.                                            */
enum { B2F_IN_NORMALIZED = 0, B2F_IN_UNIT = 1 };
B2F_API int b2f_forward_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int B, int H, int W,
                       float *dev_flow, float *dev_occ, float *dev_est3, void *stream);
/* ---- the hot path on a video: one flow per centre frame ----
 * dev_frames: T x 3 x H x W planar frames on the GPU, frame-major, H and W multiples of 64;
 * output i (i = 0 .. T-3) is what b2f_forward_device returns for the triplet of frames
 * (i, i+1, i+2), bit for bit, but the siamese feature pyramid (pwc.lua:169-211) runs once
 * per frame (T images) instead of three times (3 (T-2) images).  in_kind:
 * B2F_IN_NORMALIZED / B2F_IN_UNIT as for b2f_forward_device (fp32 samples), or B2F_IN_U8 =
 * 8-bit samples (value = byte / 255, what image.load makes of an 8-bit file) read as they
 * are, with no float copy of the frames.  Outputs (any may be NULL), planar fp32 on the GPU:
 *   dev_flow  (T-2) x 2 x H x W,  dev_occ  (T-2) x 2 x H x W,  dev_est3  (T-2) x C3 x H x W
 * (same meaning as for b2f_forward_device).  T >= 3; the shipped graph only (a context made
 * with b2f_init_ex options, two_frame among them, is refused); every device pointer
 * 16-byte aligned.  Asynchronous on `stream` like b2f_forward_device; with use_graph = 1
 * its launches are replayed from a hipGraph of their own, never one of a triplet call.   */
enum { B2F_IN_U8 = 2 };   /* sequence and f32 entries only: bytes, value = byte / 255 */
B2F_API int b2f_forward_sequence_device(b2f_ctx *ctx, const void *dev_frames, int in_kind, int T, int H, int W,
                                float *dev_flow, float *dev_occ, float *dev_est3, void *stream);
/* The same from host memory, with computeFlow's boundary (back2future.lua:47-95) around every
 * output: frames T x 3 x H0 x W0 in [0,1] (floats) or 8-bit (value = byte / 255); flow
 * (T-2) x 2 x H0 x W0 doubles, fwd_occ / bwd_occ (T-2) x H0 x W0 bytes -- output i equals
 * b2f_compute_flow(frames[i], frames[i+1], frames[i+2]).  Each frame crosses the link once
 * (the two frames a sub-batch shares with the next one twice), float frames that are all
 * k / 255 as bytes; pinned caller buffers are DMA'd in place, as in b2f_compute_flow_batch.  */
B2F_API int b2f_compute_flow_sequence(b2f_ctx *ctx, int T, const float *frames, int H0, int W0,
                              double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_u8(b2f_ctx *ctx, int T, const unsigned char *frames, int H0, int W0,
                                 double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* Several GPUs: the T-2 triplets are split with b2f_shard_range; replica i reads frames
 * [lo, hi+2) and writes outputs [lo, hi).  Same arguments and results as the single-context
 * entry points.                                                                             */
B2F_API int b2f_multi_compute_flow_sequence(b2f_multi *m, int T, const float *frames, int H0, int W0,
                                    double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_u8(b2f_multi *m, int T, const unsigned char *frames, int H0, int W0,
                                       double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* ---- float32 outputs with occlusion probabilities: computeFlow's boundary, one entry per family ----
 * The same inputs as the f64 entries above, with in_kind = B2F_IN_UNIT (floats in [0,1]) or
 * B2F_IN_U8 (bytes, value = byte / 255); B2F_IN_NORMALIZED is refused (computeFlow normalizes
 * itself).  Outputs, n = triplets (T-2 for a sequence):
 *   flow      n x 2 x H0 x W0 floats: the f64 entry's value rounded to nearest, (float)((double)f *
 *             sc) with sc_w = W0 / fw, sc_h = H0 / fh (back2future.lua:80-84); est[1] itself
 *             when H0 and W0 are multiples of 64.  Required.
 *   occ_prob  n x 2 x H0 x W0 floats or NULL: skip_occs[3] (pwc.lua:308-321, the occlusion
 *             softmax; channel c = channel c), nearest-rescaled like the masks.  For Soft models
 *             this is est[3], so fwd_occ = (occ_prob[:,1] >= 0.6666) and bwd_occ =
 *             (occ_prob[:,0] >= 0.6666).  For Hard models it is est[2], the real occlusion map,
 *             while the masks keep the reference's thresholds of est[3] -- which is the warped
 *             image 1 there -- so they are not thresholds of occ_prob.
 *   fwd_occ / bwd_occ  n x H0 x W0 bytes or NULL: the f64 entries' masks, bit for bit.
 * The kernel choice follows the caller's n as in the f64 entries, so the bits are the same.
 * Host entries: page-locked output buffers are DMA'd in place, pageable ones are copied from the
 * staging buffers; nothing is widened on the host.  A context made with b2f_init_ex options runs
 * the batch entries; the sequence entries are refused there.                                 */
B2F_API int b2f_compute_flow_batch_f32(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                               int H0, int W0, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_f32(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                  float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* Several GPUs: sharded like b2f_multi_compute_flow_batch / _sequence; every shard's kernel choice
 * follows the caller's n (the sequence rule), so the results equal one context's f32 entry.   */
B2F_API int b2f_multi_compute_flow_batch_f32(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                     int H0, int W0, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_f32(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                        float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* The same boundary on GPU memory, any H0 x W0 (frames decoded on the GPU at 1080p, ...): the
 * inputs, unpacking, image.scale to the /64 size, the forward pass and the output stage all run
 * on `stream`, asynchronously like b2f_forward_device (NULL = the context's blocking stream);
 * the results equal the f32 host entries' bit for bit.  Triplets are cut into sub-batches of
 * the host_subbatch_pixels budget (sequences overlapping by two frames) that run through a
 * workspace owned by the context: two calls on different streams must be ordered by the caller
 * (e.g. make the second stream wait for an event recorded after the first call), exactly as
 * for b2f_forward_device, whose activations live in the context too.  Every pointer must be
 * device memory (host pointers are refused) and 16-byte aligned.                              */
B2F_API int b2f_compute_flow_device(b2f_ctx *ctx, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                            int H0, int W0, float *dev_flow, float *dev_occ_prob,
                            unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
B2F_API int b2f_compute_flow_sequence_device(b2f_ctx *ctx, int T, int in_kind, const void *dev_frames, int H0, int W0,
                                     float *dev_flow, float *dev_occ_prob,
                                     unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
/* ---- flow pictures: flowX.xy2rgb(flow[1], flow[2][, max]) (flowExtensions.lua:17-150) as an output stage ----
 * The colour coding of a flow field, quantised to bytes as image.save does (floor(clip(v, 0, 1) * 255 + 0.5)):
 * hue = direction (atan(|y / x|) in degrees folded into the quadrant; x == 0: 90 for y >= 0, else 270), saturation
 * s = tanh(norm / m) with a caller-given maximum (max_norm > 0: m = max(max_norm, 1e-2)) or norm / m with the
 * automatic one (max_norm <= 0: m = max(largest norm of THAT image, 1e-2), never of the batch), lightness 1 - s / 2
 * (null flow is white), then image.hsl2rgb.  All arithmetic is fp64 on the float32 flow, without fused multiply-adds,
 * on the host and on the device, so the automatic maximum is the same double on both.
 *   flow      n x 2 x H x W floats (channel 0 = x), any H, W >= 1
 *   rgb       B2F_RGB_PLANAR: n x 3 x H x W bytes (the reference's tensor order, what image.save takes);
 *             B2F_RGB_PACKED: n x H x W x 3 bytes (what PNG / video encoders take)
 *   max_used  n doubles or NULL: the m of every image (the reference returns rgb, max)
 * Non-finite flow values give unspecified colours.                                                           */
enum { B2F_RGB_PLANAR = 0, B2F_RGB_PACKED = 1 };
/* host only, no GPU: the same per-pixel function on the CPU */
B2F_API int b2f_flow_rgb_host(const float *flow, int n, int H, int W, double max_norm, int layout,
                      unsigned char *rgb, double *max_used);
/* device pointers (16-byte aligned), asynchronous on `stream` like b2f_forward_device: after
 * b2f_compute_flow_device on the same stream it needs no synchronisation in between.  The automatic maximum is
 * reduced on the device (into dev_max_used when given, else into a buffer of the context).                  */
B2F_API int b2f_flow_rgb_device(b2f_ctx *ctx, const float *dev_flow, int n, int H, int W, double max_norm, int layout,
                        unsigned char *dev_rgb, double *dev_max_used, void *stream);
/* host pointers through the GPU, like the b2f_op_* entries below */
B2F_API int b2f_op_flow_rgb(b2f_ctx *ctx, const float *flow, int n, int H, int W, double max_norm, int layout,
                    unsigned char *rgb, double *max_used);
/* computeFlow with pictures: the f32 entries' inputs; rgb (n x 3 x H0 x W0 or n x H0 x W0 x 3 bytes) is required,
 * max_used, flow, fwd_occ and bwd_occ are optional (NULL: neither written nor downloaded).  The pictures are
 * those of b2f_op_flow_rgb on the float32 flow the f32 entries return, and the other outputs are theirs, bit for
 * bit; a caller who wants pictures downloads 3 bytes per pixel instead of 10.  Sub-batches and the multi entries'
 * shards colour every triplet from its own field, so the results do not depend on where the cuts fall.        */
B2F_API int b2f_compute_flow_batch_rgb(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                               int H0, int W0, double max_norm, int layout, unsigned char *rgb, double *max_used,
                               float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_rgb(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                  double max_norm, int layout, unsigned char *rgb, double *max_used,
                                  float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_batch_rgb(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                     int H0, int W0, double max_norm, int layout, unsigned char *rgb, double *max_used,
                                     float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_rgb(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                        double max_norm, int layout, unsigned char *rgb, double *max_used,
                                        float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* ---- scores against ground truth: the evaluation of test.lua:183-261 as an output stage ----
 * What a benchmark run does with every flow: the masked end-point error (criterions/L2Criterion.lua:36-38, times
 * flownet_factor, test.lua:190-192), the same error split by the ground truth's occlusion label (test.lua:195-223), KITTI's
 * outlier rate "Fl", and the occlusion confusion matrix behind oacc / occ_acc_* (test.lua:236-259).  Inputs per image, H x W:
 *   flow        n x 2 x H x W floats: raw network flow (what the f32 entries return)
 *   occ_prob    n x 2 x H x W floats or NULL: what the f32 entries return
 *   flow_scale  finite, > 0: pixels per unit of raw flow; 20 for the shipped models (opts.lua flownet_factor)
 *   gt_flow     n x 2 x H x W floats in pixels, as a .flo file holds them
 *   valid       n x H x W bytes or NULL: nonzero = the pixel counts (the `masks` of test.lua); NULL = every pixel
 *   gt_occ      n x H x W bytes or NULL: 0 / 1 / 2 = the labels 0 / 0.5 / 1 of test.lua:240-259 (occluded "bwd", visible,
 *               occluded "fwd"), any other byte = unlabelled
 * A pixel with valid != 0: err = |flow * flow_scale - gt_flow| in fp64 (sqrt(dy * dy + dx * dx), no fused multiply-adds), bucket
 * k = min(gt_occ, 3) (3 without gt_occ).  A NaN err adds 1 to NONFINITE and nothing else; otherwise PIXELS[k] += 1,
 * EPE_Q20[k] += (unsigned long long)(min(err, 65536) * 2^20 + 0.5), OUTLIERS[k] += (err > 3 && err > 0.05 * |gt_flow|).  Invalid
 * pixels' values enter nothing (Sintel's 1e9 marker, NaN).  With gt_occ and occ_prob, every pixel with gt_occ <= 2 -- valid or
 * not: test.lua:241-242 divides by nElement -- adds 1 to OCC[gt_occ][c], c = roundf((1 - p0) + p1) in fp32 (test.lua:236; halves
 * away from zero, NaN = 0) clamped to 0 .. 2.
 * scores: n records of B2F_SCORE_WORDS unsigned 64-bit words (176 bytes).  The sums are integers, so a record is the same words on
 * the host and on the device, whatever the order of the additions and wherever sub-batches or GPU shards are cut.  Images of
 * 2^28 pixels or more are refused (the Q20 sum could overflow).                                                              */
enum {
    B2F_SCORE_PIXELS = 0,      /* [4]  counted pixels per bucket */
    B2F_SCORE_EPE_Q20 = 4,     /* [4]  sum of the errors, 2^-20 px */
    B2F_SCORE_OUTLIERS = 8,    /* [4]  Fl outliers */
    B2F_SCORE_OCC = 12,        /* [3][3] ground-truth class major, predicted class minor */
    B2F_SCORE_NONFINITE = 21,  /* valid pixels with a NaN error */
    B2F_SCORE_WORDS = 22
};
/* host only, no GPU: test.lua:183-261 / L2Criterion.lua:36-38 per pixel on the CPU */
B2F_API int b2f_flow_score_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                        const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                        unsigned long long *scores);
/* test.lua:183-261 / L2Criterion.lua:36-38 on device pointers (16-byte aligned), asynchronous on `stream` like
 * b2f_flow_rgb_device: right behind b2f_compute_flow_device or b2f_stream_push_device on the same stream it needs no
 * synchronisation in between.  dev_scores (n x 22 words) is zeroed on the stream first.                                  */
B2F_API int b2f_flow_score_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W,
                          double flow_scale, const float *dev_gt_flow, const unsigned char *dev_valid,
                          const unsigned char *dev_gt_occ, unsigned long long *dev_scores, void *stream);
/* test.lua:183-261 / L2Criterion.lua:36-38 on host pointers through the GPU, like b2f_op_flow_rgb */
B2F_API int b2f_op_flow_score(b2f_ctx *ctx, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                      const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                      unsigned long long *scores);
/* computeFlow with scores (test.lua:183-261 / L2Criterion.lua:36-38 behind back2future.lua:47-95): the f32 entries' inputs plus
 * the ground truth, n x ... like the outputs -- record i belongs to output i, i.e. to centre frame i + 1 of a sequence.  scores
 * (n x 22 words) is required; flow, fwd_occ and bwd_occ are optional (NULL: neither written nor downloaded), so a benchmark run
 * downloads 176 bytes per triplet instead of 10 per pixel.  The scores are b2f_op_flow_score of the float32 flow and occ_prob
 * the f32 entries return, and the other outputs are theirs, bit for bit.  The ground truth is uploaded with the frames
 * (page-locked buffers in place).  A context made with b2f_init_ex options runs the batch entries; the sequence entries are
 * refused there.                                                                                                          */
B2F_API int b2f_compute_flow_batch_score(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                 int H0, int W0, double flow_scale, const float *gt_flow, const unsigned char *valid,
                                 const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                 unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_score(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                    double flow_scale, const float *gt_flow, const unsigned char *valid,
                                    const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                    unsigned char *fwd_occ, unsigned char *bwd_occ);
/* test.lua:183-261 / L2Criterion.lua:36-38 over several GPUs: sharded like the f32 entries, one context's words */
B2F_API int b2f_multi_compute_flow_batch_score(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                       int H0, int W0, double flow_scale, const float *gt_flow, const unsigned char *valid,
                                       const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                       unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_score(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                          double flow_scale, const float *gt_flow, const unsigned char *valid,
                                          const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                          unsigned char *fwd_occ, unsigned char *bwd_occ);
/* ---- motion compensation: the warped neighbours and their photometric error as an output stage ----
 * What the reference returns as warped_img_1 .. warped_img_N (back2future.lua:7-10, models/pwc.lua:67-73) and what test.lua:285
 * reports beside the EPE through criterions/OBCCriterion.lua with the L1 penalty (opts.lua:56-63: -optimize pme, OBCC, L1), at the
 * size of the caller's frames.  Inputs per image, H x W:
 *   flow        n x 2 x H x W floats: raw network flow (what the f32 entries return)
 *   occ_prob    n x 2 x H x W floats or NULL: what the f32 entries return (est[2] of a Hard model, est[3] of a Soft one)
 *   flow_scale  finite, > 0: pixels per unit of raw flow; 20 for the shipped models
 *   im1 im2 im3 past, reference and future frame, n x 3 x H x W each: B2F_IN_UNIT floats or B2F_IN_U8 bytes (value (float)k / 255.0f);
 *               they are NOT normalized
 * Direction d = 0 warps im1 with k = -(float)flow_scale, d = 1 warps im3 with k = +(float)flow_scale: the constant-velocity branch
 * of OBCCriterion.lua:79-89 (the b2f_flow_warp_past_* entries below use a Soft model's own past flow for d = 0).  The warp is nn.BilinearSamplerBHWD with CUDA semantics
 * (extras/stnbhwd/BilinearSamplerBHWD.cu:6-20,88-104) in fp32 without fused multiply-adds: xc = fx * k + (float)x, clamped to
 * [0, W - 1]; xl = floorf(xc), xw = 1 - (xc - xl); the same for y; a tap outside the image contributes 0;
 * out = (xw*yw)*tl + ((1-xw)*yw)*tr + (xw*(1-yw))*bl + ((1-xw)*(1-yw))*br, added left to right.  A pixel is inside iff
 * 0 <= xc <= W - 1 and 0 <= yc <= H - 1 before the clamp (OBCCriterion.lua:97-100, 0-based).  A NaN coordinate makes the pixel
 * non-finite for that direction: its warped value is 0 and nothing is loaded for it; +-Inf is clamped.
 * warped: n x 2 x 3 x H x W, direction major, in the frames' element type: the float value, or for bytes what image.save writes,
 * v > 0 ? (v < 1 ? (unsigned char)floorf(v * 255.0f + 0.5f) : 255) : 0.  Pixels that leave the image carry the clamped sample.
 * photo: n records of B2F_PHOTO_WORDS unsigned 64-bit words (112 bytes), word = base + d.  A finite inside pixel adds 1 to INSIDE,
 * q(e) to CHARB_Q30 with e = sum_c sqrt(dc * dc + 1e-6), dc = (double)warped_c - (double)ref_c in fp64 (L1_function.lua:20; the
 * float warp value), q(sum_c dc * dc) to SQ_Q30 and, with occ_prob, q(w * e) to OCHARB_Q30 and q(w) to WEIGHT_Q30, w = p1 for
 * d = 0 and p0 for d = 1 (OBCCriterion.lua:86,91).  A pixel with a finite coordinate that is not inside adds 1 to OUTSIDE and
 * nothing else (its error and weight are not looked at).  A NaN coordinate, or an inside pixel whose e, w * e or w is NaN, adds 1 to
 * NONFINITE and nothing else.  q(t) = (unsigned long long)(min(max(t, 0), 16) * 2^30 + 0.5).
 * The sums are integers, so a record is the same words on the host and on the device, wherever a request is cut.  Images of 2^28
 * pixels or more are refused (the Q30 sums could overflow).                                                                   */
enum {
    B2F_PHOTO_INSIDE = 0,       /* [2] finite pixels whose target lies in the image */
    B2F_PHOTO_OUTSIDE = 2,      /* [2] finite pixels whose target leaves it */
    B2F_PHOTO_CHARB_Q30 = 4,    /* [2] sum of the L1 (Charbonnier) penalties, 2^-30 */
    B2F_PHOTO_SQ_Q30 = 6,       /* [2] sum of the squared differences, 2^-30 */
    B2F_PHOTO_OCHARB_Q30 = 8,   /* [2] sum of the occlusion-weighted penalties, 2^-30 */
    B2F_PHOTO_WEIGHT_Q30 = 10,  /* [2] sum of the occlusion weights, 2^-30 */
    B2F_PHOTO_NONFINITE = 12,   /* [2] pixels with a NaN coordinate, error or weight */
    B2F_PHOTO_WORDS = 14
};
/* host only, no GPU: BilinearSamplerBHWD.cu:88-104 and OBCCriterion.lua:79-100 per pixel on the CPU.  in_kind: B2F_IN_UNIT or
 * B2F_IN_U8, the element type of im1..im3 and of warped.  warped or photo may be NULL, not both.                              */
B2F_API int b2f_flow_warp_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, int in_kind,
                       const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo);
/* BilinearSamplerBHWD.cu:88-104 / OBCCriterion.lua:79-100 on device pointers (16-byte aligned), asynchronous on `stream` like
 * b2f_flow_score_device: right behind b2f_compute_flow_device on the same stream it needs no synchronisation in between.
 * dev_photo (n x 14 words) is zeroed on the stream first.                                                                     */
B2F_API int b2f_flow_warp_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W,
                         double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                         void *dev_warped, unsigned long long *dev_photo, void *stream);
/* BilinearSamplerBHWD.cu:88-104 / OBCCriterion.lua:79-100 on host pointers through the GPU, like b2f_op_flow_score */
B2F_API int b2f_op_flow_warp(b2f_ctx *ctx, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                     int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                     unsigned long long *photo);
/* computeFlow with motion compensation (models/pwc.lua:67-73 / OBCCriterion.lua:79-100 behind back2future.lua:47-95): the f32
 * entries' inputs plus flow_scale.  warped (n x 2 x 3 x H0 x W0 in the frames' element type) and photo (n x 14 words): at least
 * one is required; flow, occ_prob, fwd_occ and bwd_occ are optional (NULL: neither written nor downloaded), so a clip's
 * photometric error costs 112 bytes of download per triplet.  Output i belongs to triplet i, i.e. to centre frame i + 1 of a
 * sequence.  The outputs are b2f_op_flow_warp of the float32 flow and occ_prob the f32 entries return and of the caller's own
 * frames, bit for bit, and the other outputs are the f32 entries'.  A context made with b2f_init_ex options runs the batch
 * entries; the sequence entries are refused there.  Streams have no such entry (their frame slots hold rescaled frames).     */
B2F_API int b2f_compute_flow_batch_warp(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                int H0, int W0, double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_warp(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                   double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                   float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* models/pwc.lua:67-73 / OBCCriterion.lua:79-100 over several GPUs: sharded like the f32 entries, one context's bytes and words */
B2F_API int b2f_multi_compute_flow_batch_warp(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                      int H0, int W0, double flow_scale, void *warped, unsigned long long *photo,
                                      float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_warp(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                         double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                         float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* ---- the past flow of the Soft models: skip_ubfs[3], and motion compensation with it ----
 * A Soft model estimates two flows per reference frame (opts.lua:58 "Jointly predict future and past flow"): the future flow
 * skip_ufs, which every entry above returns as `flow`, and the past flow skip_ubfs of its own decoder chain (models/pwc.lua:328-385).
 * The reference warps the past frame with the past flow (pwc.lua:425-432) and forms the past half of the photometric error with it
 * (criterions/OBCCriterion.lua:80-81).  The entries below return it beside the other outputs: `past_flow` (dev_past_flow) stands
 * after `flow` and is otherwise like it -- n x 2 x H x W floats, a RAW network flow (pixels / 20 for the shipped models), at
 * H0 x W0 (float)((double)f * sc) with the nearest-index rule of image.scale(..., 'simple'), the network's own planes at /64 sizes.
 * Sign: the past frame is sampled at x - past_flow * flow_scale, as the future frame is sampled at x + flow * flow_scale; under
 * constant velocity past_flow == flow.  A NULL past_flow is neither computed nor downloaded and the call is the entry's without
 * the suffix; with it the pruned forward pass also runs the five past-flow decoders, and every other output keeps its bits.
 * A context without past-flow decoders (a Hard model, two_frame) is refused, and so is a stream that was not opened with
 * B2F_STREAM_PAST (b2f_stream_open_ex, b2f_stream_push_past); a refusal launches nothing.                                        */
B2F_API int b2f_forward_device_past(b2f_ctx *ctx, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow,
                            float *dev_past_flow, float *dev_occ, float *dev_est3, void *stream);
B2F_API int b2f_forward_sequence_device_past(b2f_ctx *ctx, const void *dev_frames, int in_kind, int T, int H, int W, float *dev_flow,
                                     float *dev_past_flow, float *dev_occ, float *dev_est3, void *stream);
B2F_API int b2f_compute_flow_batch_past(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                int H0, int W0, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_past(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0, float *flow,
                                   float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_device_past(b2f_ctx *ctx, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                                 int H0, int W0, float *dev_flow, float *dev_past_flow, float *dev_occ_prob,
                                 unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
B2F_API int b2f_compute_flow_sequence_device_past(b2f_ctx *ctx, int T, int in_kind, const void *dev_frames, int H0, int W0,
                                          float *dev_flow, float *dev_past_flow, float *dev_occ_prob,
                                          unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
B2F_API int b2f_multi_compute_flow_batch_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                      int H0, int W0, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                      unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, float *flow,
                                         float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* Motion compensation with the model's own past flow: everything is b2f_flow_warp_* above except that direction d = 0 takes its
 * coordinate from past_flow: xc = past_fx * k + (float)x with k = -(float)flow_scale, and inside / outside / non-finite are
 * decided on that coordinate; the weights stay p1 / p0, the record layout stays B2F_PHOTO_*.  With past_flow == flow every byte
 * and word is b2f_flow_warp_*'s.  On normalized frames the d = 0 planes are the reference's warped_img_1 of a Soft model.  The
 * compute_flow forms take the outputs of the _warp entries plus the optional past_flow output: the past flow is produced on the
 * device whenever such a request arrives and downloaded only when asked for.                                                   */
B2F_API int b2f_flow_warp_past_host(const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W,
                            double flow_scale, int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                            unsigned long long *photo);
B2F_API int b2f_flow_warp_past_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_past_flow, const float *dev_occ_prob, int n,
                              int H, int W, double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2,
                              const void *dev_im3, void *dev_warped, unsigned long long *dev_photo, void *stream);
B2F_API int b2f_op_flow_warp_past(b2f_ctx *ctx, const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W,
                          double flow_scale, int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                          unsigned long long *photo);
B2F_API int b2f_compute_flow_batch_warp_past(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                     int H0, int W0, double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                     float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_compute_flow_sequence_warp_past(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                        double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                        float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_batch_warp_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                           int H0, int W0, double flow_scale, void *warped, unsigned long long *photo,
                                           float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                           unsigned char *bwd_occ);
B2F_API int b2f_multi_compute_flow_sequence_warp_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                              double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                              float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                              unsigned char *bwd_occ);
/* ---- the unsupervised validation loss: the -optimize pme branch of test.lua:266-297 on the output table ----
 * What the reference validates a model trained without labels with: on every level j = 0 .. L-1 of the output table of model:forward
 * (pwc.lua:459-489; level size h = H >> j, w = W >> j) the contrast-sensitive smoothness of the flows
 * (criterions/SmoothnessCriterion.lua:45-63), the constant-velocity term (criterions/ConstVelCriterion.lua:36-38), the occlusion-aware
 * photometric error of the table's own warped images (criterions/OBCCriterion.lua:79-100), the smoothness of the occlusions
 * (os_criterion, model.lua:216) and the occlusion prior (criterions/OcclusionPriorCriterion.lua:39).  Inputs per level, planar fp32:
 * f the future flow (2 channels), p the past flow (2, Soft tables only), o the occlusions (2), iw1 / iw3 the warped images (3 each),
 * R_j the reference image (3): R_0 = the normalized centre frame, R_j = the 2 x 2 mean of R_{j-1} in fp32,
 * (((tl + tr) + bl) + br) / 4 (nn.SpatialAveragePooling(2,2,2,2), test.lua:132,269).  All per-pixel arithmetic is fp64 without fused
 * multiply-adds (the warp coordinate fp32):
 *   dx(F,c) = (double)F[c][y][x+1] - (double)F[c][y][x] if x + 1 < w, else 0; dy the same over rows
 *   wx = E(-20 * ((|dx(R,0)| + |dx(R,1)|) + |dx(R,2)|) / 3.0), wy the same with dy (SmoothnessCriterion.lua:58-59, cs = 20)
 *   E(t), t <= 0: the library's own exponential -- t > 0 counts as 0, t < -708 gives 0, NaN stays NaN;
 *        k = nearbyint(t * 1.44269504088896338700e+00), r = (t - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10,
 *        p = c13, p = p * r + c_i for i = 12 .. 0 with c_0 = 1, c_i = c_{i-1} / i; E = ldexp(p, k)
 *   P1(v) = sqrt(v * v + 1e-6) (L1_function.lua:20), P2(v) = v * v
 *   s_flow = (P1(dx(f,0)) * wx + P1(dy(f,0)) * wy) + (P1(dx(f,1)) * wx + P1(dy(f,1)) * wy); s_past the same on p; s_occ the same with
 *            P2 on o; cv = sqrt(d0 * d0 + d1 * d1), d_c = (double)f[c] - (double)p[c]; prior = 1.0 - (double)o[0] * (double)o[1]
 * Each term adds q(term) to its word, q(t) = (unsigned long long)(min(max(t, 0), 16) * 2^30 + 0.5); a NaN term adds nothing and its
 * pixel counts once in NONFINITE.  Photo words, direction d = 0 the past frame iw1, d = 1 the future frame iw3: the pixel's target is
 * that of b2f_flow_warp with k_0 = -(float)(flow_scale / 2^j), k_1 = +(float)(flow_scale / 2^j) (pwc.lua:450-455, train.lua:425) on the
 * past flow for d = 0 of a Soft table (OBCCriterion.lua:80-81) and on the future flow otherwise; INSIDE / OUTSIDE / OCHARB_Q30 /
 * PHOTO_NONFINITE are the B2F_PHOTO_* words of that pixel with the warped value iw_d, the reference R_j and the weight o[1] (d = 0) or
 * o[0] (d = 1).
 * loss: n x L records of B2F_LOSS_WORDS unsigned 64-bit words (128 bytes), image-major.  The sums are integers, so a record is the same
 * words on the host and on the device, wherever a request is cut.  Images of 2^28 pixels or more are refused; L is 1 .. 7; H and W
 * are multiples of 2^(L-1).                                                                                                     */
enum {
    B2F_LOSS_PIXELS = 0,            /* h * w */
    B2F_LOSS_SMOOTH_FLOW_Q30 = 1,   /* flow smoothness of the future flow, 2^-30 */
    B2F_LOSS_SMOOTH_PAST_Q30 = 2,   /* flow smoothness of the past flow (0 for Hard) */
    B2F_LOSS_CONST_VEL_Q30 = 3,     /* constant-velocity term (0 for Hard) */
    B2F_LOSS_SMOOTH_OCC_Q30 = 4,    /* occlusion smoothness */
    B2F_LOSS_PRIOR_OCC_Q30 = 5,     /* occlusion prior */
    B2F_LOSS_PHOTO_INSIDE = 6,      /* [2] finite pixels whose target lies in the image, past / future */
    B2F_LOSS_PHOTO_OUTSIDE = 8,     /* [2] finite pixels whose target leaves it */
    B2F_LOSS_PHOTO_OCHARB_Q30 = 10, /* [2] occlusion-weighted Charbonnier error */
    B2F_LOSS_PHOTO_NONFINITE = 12,  /* [2] non-finite photo pixels */
    B2F_LOSS_NONFINITE = 14,        /* pixels with a NaN smoothness, velocity or prior term */
    B2F_LOSS_WORDS = 16             /* word 15 is reserved, always 0 */
};
/* host only, no GPU: test.lua:266-297 per pixel on the CPU.  table: n_outs = L * (4 + past_flow) pointers in table order (per level
 * f, [p,] o, iw1, iw3; shapes as b2f_output_shapes gives them); ref: n x 3 x H x W; loss: n x L x 16 words.                     */
B2F_API int b2f_table_loss_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                        double flow_scale, unsigned long long *loss);
/* test.lua:266-297 on device pointers: dev_table is a host array of n_outs device pointers (16-byte aligned, as dev_ref and
 * dev_loss); n_outs = 4 L (Hard) or 5 L (Soft), past_flow is taken from it with the context's kind (20 = 4 x 5 = 5 x 4 is read as
 * the context's).  Asynchronous on `stream` like b2f_flow_warp_device; dev_loss (n x L x 16 words) is zeroed on the stream first.
 * The pyramid of R lives in a workspace of the context: calls on different streams must be ordered by the caller.  At most 65535
 * images per call.                                                                                                              */
B2F_API int b2f_table_loss_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                          double flow_scale, unsigned long long *dev_loss, void *stream);
/* test.lua:266-297 on host pointers through the GPU, like b2f_op_flow_warp */
B2F_API int b2f_op_table_loss(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                      double flow_scale, unsigned long long *loss);
/* model:forward followed by test.lua:266-297 without the download of the table: x is n x 9 x H x W normalized host memory (H, W as
 * for b2f_forward), ref is its channels 3 .. 5; loss: n x L x 16 words with L = b2f_info's n_outputs / (4 | 5).  outs = NULL with
 * n_outs = 0: the table stays on the device and the call returns n x L x 128 bytes; otherwise outs receives the table, bit for bit
 * that of b2f_forward.  Requests are cut into sub-batches of the host_subbatch_pixels budget; the table lives in a workspace of the
 * context.  A context made with b2f_init_ex options is served wherever its table has occlusions; two_frame is refused.         */
B2F_API int b2f_forward_loss(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                     float **outs, int n_outs);
/* test.lua:266-297 behind model:forward on device pointers: dev_in n x 9 x H x W, in_kind B2F_IN_NORMALIZED only; dev_loss
 * n x L x 16 words; asynchronous on `stream` like b2f_forward_device.                                                           */
B2F_API int b2f_forward_loss_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                            unsigned long long *dev_loss, void *stream);
/* test.lua:266-297 over several GPUs: the n triplets are split with b2f_shard_range; one context's words */
B2F_API int b2f_multi_forward_loss(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss);
/* ---- the fine-tuning objective of the Soft models: the terms of README.md:89-102 beside those above ----
 * Ours-Soft-ft-KITTI and Ours-Soft-ft-Sintel were trained with -smooth_second_order and -pme_criterion OBGCC.  The *_ft entries
 * return records of 24 words per image and level: words 0 .. 15 are those of the entries above, bit for bit, and words 16 .. 23 carry
 * the second-order smoothness (criterions/SecondOrderSmoothnessCriterion.lua:45-65) and the gradient-constancy sums of
 * criterions/OBGCCriterion.lua:67-68,91-105, both with the L1 penalty P1.  Same inputs, same fp64 arithmetic without fused
 * multiply-adds, same E, P1 and q as above.  Per pixel (x, y) of a level of h x w, a missing neighbour giving no term (so levels
 * the reference cannot slice, h < 3 or w < 3, are defined too):
 *   gx(F,c) = (2.0 * F[c][y][x] - F[c][y][x-1]) - F[c][y][x+1] if 0 < x and x + 1 < w, else 0; gy the same over rows
 *   m(a, b) = ((|R0(a) - R0(b)| + |R1(a) - R1(b)|) + |R2(a) - R2(b)|) / 3.0
 *   igx = (x > 0 ? m((x,y), (x-1,y)) : 0) + (0 < x and x + 1 < w ? m((x,y), (x+1,y)) : 0); igy the same over rows (lines 55-58)
 *   wx = E(-20.0 * igx), wy = E(-20.0 * igy)
 *   the four products of a flow F: P1(gx(F,0)) * wx, P1(gy(F,0)) * wy, P1(gx(F,1)) * wx, P1(gy(F,1)) * wy: a border pixel adds
 *           P1(0) = 1e-3 times its weight, not 0 (lines 38-39 zero the second differences, line 65 applies the penalty to them)
 * SMOOTH2_FLOW_Q30 sums q of each of the four products of f, SMOOTH2_PAST_Q30 of p (0 for Hard): q saturates at 16, which a sum of
 * products could reach and one product of a plausible flow cannot.  If a product of a flow is NaN the pixel adds nothing for that flow
 * and counts once in SMOOTH2_NONFINITE.  Gradient constancy, direction d as above with its warped image I = iw_d and weight o[1 - d]:
 *   dx_c = (I[c][y][x+1] - I[c][y][x]) - (R[c][y][x+1] - R[c][y][x]) if x + 1 < w, else 0 (lines 67-68, 91-92: both forward
 *          differences are 0 in the last column); dy_c the same over rows
 * A pixel-direction that counts in PHOTO_INSIDE adds (q(o * P1(dx_0)) + q(o * P1(dx_1))) + q(o * P1(dx_2)) to PHOTO_OGX_Q30[d] and
 * the same with dy to PHOTO_OGY_Q30[d] (per channel: the three-channel sum of normalized images can pass q's saturation at 16, one
 * channel cannot); if any of the six products is NaN it adds to neither and counts in GRAD_NONFINITE.  Any other pixel-direction
 * adds nothing.  The brightness part of OBGCC is PHOTO_OCHARB_Q30: line 97 never applies alpha to it, only beta and gamma weigh the
 * two gradient sums (back2future.loss_summary).  The words are macros, below the entries: the enumeration above stays as it is.  */
/* The six entries above with records of 24 words (192 bytes): same arguments, same checks, same sub-batching, same workspaces. */
B2F_API int b2f_table_loss_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                           double flow_scale, unsigned long long *loss);
B2F_API int b2f_table_loss_ft_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                             double flow_scale, unsigned long long *dev_loss, void *stream);
B2F_API int b2f_op_table_loss_ft(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                         double flow_scale, unsigned long long *loss);
B2F_API int b2f_forward_loss_ft(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                        float **outs, int n_outs);
B2F_API int b2f_forward_loss_ft_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                               unsigned long long *dev_loss, void *stream);
B2F_API int b2f_multi_forward_loss_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss);
#define B2F_LOSS_FT_SMOOTH2_FLOW_Q30 16   /* second-order smoothness of the future flow, 2^-30 */
#define B2F_LOSS_FT_SMOOTH2_PAST_Q30 17   /* second-order smoothness of the past flow (0 for Hard) */
#define B2F_LOSS_FT_PHOTO_OGX_Q30 18      /* [2] occlusion-weighted gradient-constancy error in x, past / future */
#define B2F_LOSS_FT_PHOTO_OGY_Q30 20      /* [2] the same in y */
#define B2F_LOSS_FT_SMOOTH2_NONFINITE 22  /* pixels with a NaN second-order term */
#define B2F_LOSS_FT_GRAD_NONFINITE 23     /* pixel-directions of PHOTO_INSIDE with a NaN gradient term */
#define B2F_LOSS_FT_WORDS 24
/* ---- the gradient of the pme objective with respect to the output table: `gradOutputs` of train.lua:279-472 ----
 * What the fine-tuning commands of README.md:85-102 hand to model:backward: a table with the shapes of the output table, into which
 * every criterion's backward, times its option weight and level_weights[l], is added (train.lua:428-468).  The scope is -optimize
 * pme with the defaults of opts.lua: SmoothnessCriterion with the L1 penalty for the flows and the quadratic one for the
 * occlusions, ConstVelCriterion, OBCCriterion with L1, OcclusionPriorCriterion -- the objective of Ours-Hard.  The gradients of
 * SecondOrderSmoothnessCriterion and OBGCCriterion (the *_ft entries' two criteria) are those of the *_grad_ft entries below.
 * The specification is the reference's updateGradInput functions, not the mathematical derivative of their outputs; they differ in
 * three places, all kept:
 *   1. OcclusionPriorCriterion.lua:64-65 returns 1 - o[other]; the derivative of 1 - o0 * o1 is -o[other].  The value is larger by
 *      the constant k_pr on both channels, which the softmax below the occlusions cancels.
 *   2. OBCCriterion.lua:181-182,210-211: a pixel-direction whose target leaves the image adds penalty_out = 1 to the occlusion
 *      gradient of channel 1 - d; the forward value has a constant there.
 *   3. ConstVelCriterion.lua:69-70 divides the gradient by h w with sizeAverage, line 33 the output by 2 h w.
 * Inputs, R_j, dx, dy, wx, wy, E, P1 and the direction's target (`inside` of b2f_flow_warp's coordinate, fp32; a NaN coordinate is
 * not inside, as Lua's comparisons decide) are those of the loss records above; all other arithmetic is fp64 without fused
 * multiply-adds.  With D1(v) = v / sqrt(v * v + 1e-6), D2(v) = 2.0 * v, per level j of h x w and c_j = level_weights[j]:
 *   a(F,D)(x,y) = D(dx(F)(x,y)) * wx(x,y) where x + 1 < w, otherwise exactly 0 (no multiplication by a weight); b the same over rows
 *   S(F,D)(x,y) = (((-a(x,y)) + a(x-1,y)) - b(x,y)) + b(x,y-1), a term with x - 1 < 0 or y - 1 < 0 being 0
 *   d_c = (double)f[c] - (double)p[c], CV_c = d_c / (sqrt(d0 * d0 + d1 * d1) + 1e-12)
 *   direction d (0: iw1, the target on the past flow of a Soft table, weight o[1]; 1: iw3, weight o[0]): m_d = inside,
 *   delta_c = (double)iw_d[c] - (double)R_j[c], e_d = (P1(delta_0) + P1(delta_1)) + P1(delta_2), PO_{1-d} = m_d ? e_d : 1.0
 *   k_s = (c_j * smooth_flow) * N2, k_cv = (c_j * const_vel) * N1, k_p = ((c_j * pme) * N1) / 6.0, k_so = (c_j * smooth_occ) * N2,
 *   k_pr = (c_j * prior_occ) * N1; N2 = 1.0 / ((2.0 * h) * w) and N1 = 1.0 / ((double)h * w) with size_average (per triplet, as
 *   back2future.loss_summary(size_average=True) counts), otherwise 1
 *   G_f[c]    = k_s * S(f[c],D1) + k_cv * CV_c                       (the second term on Soft tables only)
 *   G_p[c]    = k_s * S(p[c],D1) - k_cv * CV_c                       (Soft tables only)
 *   G_o[c]    = (k_p * PO_c + k_so * S(o[c],D2)) + k_pr * (1.0 - (double)o[1-c])
 *   G_iw_d[c] = m_d ? k_p * (D1(delta_c) * (double)o[1-d]) : +0.0
 * A term whose option weight is exactly 0 is not evaluated and adds nothing (train.lua:458,465 do this for the two occlusion terms;
 * here all five): the remaining terms are added left to right, an element without one is +0.0.  Everything else follows IEEE: a
 * NaN input gives NaN in the elements that read it.  Every element is summed in fp64 and rounded to fp32 once, on store, so the
 * host entry and the kernel give the same bits; the reference accumulates in fp32 and rounds after every add.
 * The gradient table has the output table's n_outs tensors and shapes; it must not alias the table or ref.                      */
typedef struct b2f_loss_grad_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;   /* opts.lua:61-73; each finite and >= 0 */
    double level_weights[7];                                     /* test.lua:29-31; each finite and >= 0 */
    int size_average;                                            /* the criteria's sizeAverage, per triplet */
} b2f_loss_grad_opts;
/* opts.lua:61-73 (1, 1, 1, 0.1, 0.1), test.lua:29-31 (0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28), size_average = 0 */
B2F_API int b2f_loss_grad_defaults(b2f_loss_grad_opts *opts);
/* host only, no GPU.  table, n_outs, past_flow, ref as for b2f_table_loss_host; opts = NULL: the defaults; grad: n_outs pointers
 * to tensors of the table's shapes.                                                                                             */
B2F_API int b2f_table_loss_grad_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                             double flow_scale, const b2f_loss_grad_opts *opts, float *const *grad);
/* on device pointers: dev_table and dev_grad are host arrays of n_outs device pointers (16-byte aligned, as dev_ref); checks,
 * stream and the pyramid's workspace as for b2f_table_loss_device.  Every element of dev_grad is written.                        */
B2F_API int b2f_table_loss_grad_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                               const float *dev_ref, double flow_scale, const b2f_loss_grad_opts *opts, float *const *dev_grad,
                               void *stream);
/* on host pointers through the GPU, like b2f_op_table_loss */
B2F_API int b2f_op_table_loss_grad(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                           double flow_scale, const b2f_loss_grad_opts *opts, float *const *grad);
/* model:forward followed by the gradient table: x as for b2f_forward_loss; grad: n_outs = b2f_info's n_outputs host tensors of the
 * output table's shapes.  loss (optional, NULL: none): the n x L x 16 words of b2f_forward_loss, from the same pyramid; outs
 * (optional, NULL: none): n_outs tensors that receive the table, bit for bit that of b2f_forward.  Sub-batches and workspaces as
 * for b2f_forward_loss; two_frame is refused.                                                                                   */
B2F_API int b2f_forward_loss_grad(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_opts *opts,
                          unsigned long long *loss, float *const *grad, int n_outs, float *const *outs);
/* the same on device pointers: dev_in n x 9 x H x W, in_kind B2F_IN_NORMALIZED only; dev_loss optional; dev_grad a host array of
 * n_outs device tensors for all n triplets; asynchronous on `stream` like b2f_forward_loss_device.                               */
B2F_API int b2f_forward_loss_grad_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                 const b2f_loss_grad_opts *opts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs,
                                 void *stream);
/* b2f_forward_loss_grad over several GPUs: the n triplets are split with b2f_shard_range; one context's bits */
B2F_API int b2f_multi_forward_loss_grad(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                const b2f_loss_grad_opts *opts, unsigned long long *loss, float *const *grad, int n_outs);
/* ---- the gradient of the Soft models' fine-tuning objective with respect to the output table ----
 * Ours-Soft-ft-KITTI and Ours-Soft-ft-Sintel were fine-tuned with -smooth_second_order -pme_criterion OBGCC (README.md:89-102).  The
 * *_grad_ft entries are the *_grad entries above with two terms of a level replaced where their flag is set; everything not named
 * here -- inputs, coefficients, CV_c, S(o[c],D2), the prior, the rule for a weight of exactly 0, one rounding to fp32 on store -- is as
 * above, and with both flags 0 every element is the expression above, bit for bit.  The specification is again updateGradInput:
 * criterions/SecondOrderSmoothnessCriterion.lua:77-104 and criterions/OBGCCriterion.lua:151-300, both with the L1 penalty.
 * smooth_second_order: S(f[c],D1) and S(p[c],D1) become S2(f[c]) and S2(p[c]).  With gx, gy, m and E of the *_ft records above:
 *   wx(x,y) = E(-20.0 * (m((x,y), (x-1,y)) + m((x,y), (x+1,y)))) and qx(F)(x,y) = D1(gx(F)(x,y)) * wx(x,y) where 0 < x and x + 1 < w;
 *   elsewhere qx is not formed and counts as +0.0; wy, qy the same over rows (a map with w < 3 or h < 3 has no term on that axis,
 *   the per-pixel rule of the records; the Lua slices cannot express it)
 *   S2(F)(x,y) = (((((2.0 * qy(x,y)) + (2.0 * qx(x,y))) - qy(x,y+1)) - qx(x+1,y)) - qy(x,y-1)) - qx(x-1,y)      (lines 92-97)
 *   G_f[c] = k_s * S2(f[c]) + k_cv * CV_c, G_p[c] = k_s * S2(p[c]) - k_cv * CV_c
 * pme_criterion = 1 (OBGCC): per direction d with I = iw_d, R = R_j, m_d and the weight o[1-d] as above, per channel c
 *   delta_c = (double)I[c] - (double)R[c]; ex_c = dx_c and ey_c = dy_c of the *_ft records (0 in the last column / row)
 *   T(F) = the enabled ones of  alpha * F(delta), -(gamma * F(ey(x,y))), gamma * F(ey(x,y-1)), -(beta * F(ex(x,y))),
 *          beta * F(ex(x-1,y))  added left to right; the third only where y > 0, the fifth only where x > 0; a term whose weight
 *          alpha, beta or gamma is exactly 0 is not evaluated; +0.0 without a term
 *   G_iw_d[c] = m_d ? k_p * (T(D1 of channel c) * (double)o[1-d]) : +0.0
 *   PO_{1-d}  = m_d ? T(v -> (P1(v_0) + P1(v_1)) + P1(v_2), the sum over the three channels) : 1.0
 * alpha = 1, beta = gamma = 0 give OBCC's bits.  Four more places where the gradient is not the derivative of the records' value,
 * all kept:
 *   1. alpha multiplies the gradient (lines 202, 215); updateOutput never applies it (line 97).
 *   2. Lines 207 and 212 add the neighbour's derivative D1(ey(x,y-1)), D1(ex(x-1,y)) to the pixel (x,y) before lines 246 and 254
 *      mask and weigh it: with the pixel's own m_d and o[1-d], where the derivative has the neighbour's.
 *   3. Lines 215-219 build the occlusion gradient from the penalty's values with the derivative's signs, so PO is not the pixel's
 *      error e_d + beta ... ; in the last column and row, where ex / ey is 0, it subtracts P1(0) = 1e-3 per channel.
 *   4. model.lua:171 writes -pme_gamma into a field named `gamm`, so a reference run keeps gamma = 1; the option is honoured here as
 *      given (back2future.LOSS_OBJECTIVES).
 * (The Lua accumulates the warped images' forward differences over the two directions, lines 194-195 without a reset; like the
 * records, each direction takes its own image here.)                                                                             */
typedef struct b2f_loss_grad_ft_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;   /* as b2f_loss_grad_opts */
    double level_weights[7];
    int size_average;
    int smooth_second_order;                                     /* -smooth_second_order: 0 | 1 */
    int pme_criterion;                                           /* -pme_criterion: 0 OBCC, 1 OBGCC */
    double pme_alpha, pme_beta, pme_gamma;                       /* OBGCC's weights; each finite and >= 0 */
} b2f_loss_grad_ft_opts;
/* b2f_loss_grad_defaults, smooth_second_order = 1, pme_criterion = 1, alpha = beta = gamma = 1 */
B2F_API int b2f_loss_grad_ft_defaults(b2f_loss_grad_ft_opts *opts);
/* The six entries above with these options: same arguments, same checks (and pme_criterion in {0, 1}), same sub-batching, same
 * workspaces; a refusal writes nothing.  The optional records of the two forward entries are the 24 words of b2f_forward_loss_ft. */
B2F_API int b2f_table_loss_grad_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                double flow_scale, const b2f_loss_grad_ft_opts *opts, float *const *grad);
B2F_API int b2f_table_loss_grad_ft_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                  const float *dev_ref, double flow_scale, const b2f_loss_grad_ft_opts *opts,
                                  float *const *dev_grad, void *stream);
B2F_API int b2f_op_table_loss_grad_ft(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                              double flow_scale, const b2f_loss_grad_ft_opts *opts, float *const *grad);
B2F_API int b2f_forward_loss_grad_ft(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                             const b2f_loss_grad_ft_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                             float *const *outs);
B2F_API int b2f_forward_loss_grad_ft_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                    const b2f_loss_grad_ft_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                    int n_outs, void *stream);
B2F_API int b2f_multi_forward_loss_grad_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                   const b2f_loss_grad_ft_opts *opts, unsigned long long *loss, float *const *grad, int n_outs);
/* ---- the occlusion-aware SSIM + L1 photometric term: -pme_criterion OSSIM | OSSIML1 (opts.lua:62, model.lua:172-179) ----
 * criterions/OSSIML1Criterion.lua:47-163 beside the terms above.  The *_ssim entries return records of 32 words per image and level:
 * words 0 .. 15 are those of b2f_table_loss*, bit for bit, words 16 .. 25 the sums below, words 26 .. 31 are 0.  Same inputs, same fp64
 * arithmetic without fused multiply-adds, same P1 and q.  Per level j of h x w, image by image:
 *   range: (mn, mx), two floats, from range_mode --
 *     B2F_SSIM_RANGE_BATCH  the minimum and maximum over R_j, iw1 and iw3 of all n images of the call (lines 62-67: the reference's);
 *                           a record then depends on the other images of its call, so the b2f_forward_loss_ssim* entries refuse
 *                           it when the request would be cut into more than one sub-batch, and b2f_multi_forward_loss_ssim always
 *     B2F_SSIM_RANGE_IMAGE  the image's own minimum and maximum (the reference's at batch size 1)
 *     B2F_SSIM_RANGE_GIVEN  ranges[2 j], ranges[2 j + 1]: `ranges` is a host array of L x 2 floats (NULL in the other modes)
 *     NaNs are skipped, infinities kept, -0 < +0.  The image's own pair is returned in words 24 / 25 in every mode, the pair used in
 *     words 22 / 23, as float bits.
 *   t(v) = ((double)v - (double)mn) / ((double)mx - (double)mn)
 *   window: G(a)(x, y) = (ge * col(x-1) + gc * col(x)) + ge * col(x+1), col(x') = (ge * a(x', y-1) + gc * a(x', y)) + ge * a(x', y+1),
 *     indices clamped to the plane (SpatialReplicationPadding(1), lines 38-44), so that 1 x 1, 1 x w and h x 1 levels are defined;
 *     e = exp(-8/9), ge = e / (1 + 2 e), gc = 1 / (1 + 2 e): image.gaussian{size = 3, normalize = true} as restated in
 *     csrc/b2f_tableloss_ssim.h, which says where the weights come from (b2f_loss_ssim_weights returns ge, gc)
 *   per direction d (0 the past frame iw1, 1 the future frame iw3) and channel c, x = t(iw_d[c]), y = t(R_j[c]):
 *     mu_x = G(x), mu_y = G(y), s_x = G(x * x) - mu_x * mu_x, s_y = G(y * y) - mu_y * mu_y, s_xy = G(x * y) - mu_x * mu_y
 *     l = (2.0 * (mu_x * mu_y) + 1e-4) / ((mu_x * mu_x + mu_y * mu_y) + 1e-4), cs = (2.0 * s_xy + 9e-4) / ((s_x + s_y) + 9e-4)
 *     S = ((1.0 - l * cs)_0 + (..)_1) + (..)_2, B = (P1(x_0 - y_0) + P1(x_1 - y_1)) + P1(x_2 - y_2)
 * A pixel-direction that counts in PHOTO_INSIDE adds q(o * S) to SSIM_Q30[d] and q(o * B) to L1N_Q30[d], o = o[1 - d] as above
 * (S <= 6 and B <= 3 sqrt(1 + 1e-6) on a range that holds the values: q cannot saturate).  If either product is NaN, or the range is
 * unusable (not mx > mn, or either not finite), it adds to neither and counts in SSIM_NONFINITE[d].  Any other pixel-direction adds
 * nothing: OUTSIDE and the occlusion weight are those of OBCCriterion (lines 121-151 against OBCCriterion.lua:78-105).  The criterion's
 * value is sum over d of ((alpha * SSIM_d + (1 - alpha) * L1N_d) / 2^30 + OUTSIDE_d) / (3 * 2) with alpha = 1 (OSSIM) or 0.85 (OSSIML1)
 * (back2future.loss_summary).  updateGradInput is that of the *_grad_ssim entries below.                                      */
/* The six b2f_*_loss_ft entries with records of 32 words (256 bytes) and the range: same checks, same sub-batching, same workspaces. */
B2F_API int b2f_table_loss_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                             double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
B2F_API int b2f_table_loss_ssim_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                               double flow_scale, unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_op_table_loss_ssim(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                           double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_ssim(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                          float **outs, int n_outs, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_ssim_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                 unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_multi_forward_loss_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                                int range_mode, const float *ranges);
/* out[0] = ge, out[1] = gc: the 1-D weights of the window */
B2F_API int b2f_loss_ssim_weights(double out[2]);
#define B2F_SSIM_RANGE_BATCH 0          /* range_mode: the minimum and maximum over the n images of the call */
#define B2F_SSIM_RANGE_IMAGE 1          /* each image's own */
#define B2F_SSIM_RANGE_GIVEN 2          /* ranges[2 j], ranges[2 j + 1] */
#define B2F_LOSS_SSIM_Q30 16           /* [2] occlusion-weighted sum over the channels of 1 - l * cs, past / future, 2^-30 */
#define B2F_LOSS_SSIM_L1N_Q30 18       /* [2] occlusion-weighted L1 penalty of the range-normalised difference */
#define B2F_LOSS_SSIM_NONFINITE 20     /* [2] pixel-directions of PHOTO_INSIDE with a NaN product or an unusable range */
#define B2F_LOSS_SSIM_RANGE_USED 22    /* [2] float bits, zero-extended, of the mn / mx used for this image and level */
#define B2F_LOSS_SSIM_RANGE_OWN 24     /* [2] float bits of this image's own minimum / maximum at this level */
#define B2F_LOSS_SSIM_WORDS 32         /* words 26 .. 31 are reserved, always 0 */
/* ---- the gradient of the SSIM + L1 photometric term with respect to the output table (b2f_version() >= 1011) ----
 * The *_grad_ssim entries are the *_grad_ft entries above with the photometric term of a level replaced by that of
 * criterions/OSSIML1Criterion.lua:165-302 (updateGradInput), combined with the other terms as train.lua:428-468 does.  Everything
 * not named here -- inputs, R_j, m_d (the past flow for d = 0 on Soft tables), the coefficients k_*, N1, N2, CV_c, S, S2, the prior,
 * the rule for a weight of exactly 0, the range (mn, mx) with its three modes, t(v), the window G in its fixed order, ge, gc, C1 =
 * 1e-4, C2 = 9e-4, P1, D1, fp64 without fused multiply-adds, one rounding to fp32 on store -- is as stated above.  Per level,
 * direction d and channel c, with x = t(iw_d[c]), y = t(R_j[c]) and the five window sums mu_x, mu_y, gxx = G(x x), gyy = G(y y),
 * gxy = G(x y):
 *   xx = mu_x * mu_x, yy = mu_y * mu_y, xy = mu_x * mu_y; s_x = gxx - xx, s_y = gyy - yy, s_xy = gxy - xy
 *   A = (xx + yy) + C1, Bd = (s_x + s_y) + C2; l = (2.0 * xy + C1) / A, cs = (2.0 * s_xy + C2) / Bd
 *   gw = gc * gc                                                       (the window's centre tap, lines 204, 216)
 *   dl = ((2.0 * gw) * (mu_y - mu_x * l)) / A                           (line 217)
 *   dcs = ((2.0 * gw) * ((y - mu_y) - cs * (x - mu_x))) / Bd            (line 218)
 *   Q_c = dl * cs + l * dcs
 *   T_c = the enabled ones of  -(alpha * Q_c),  (1.0 - alpha) * D1(x - y)  added left to right; alpha == 0 resp. (1.0 - alpha) == 0:
 *         not evaluated; +0.0 without a term
 *   G_iw_d[c] = m_d ? k_p * (T_c * (double)o[1-d]) : +0.0
 *   PO_{1-d}  = m_d ? (the enabled ones of alpha * S, (1.0 - alpha) * B, with S and B of the records above) : 1.0
 *   G_o[c]    = (k_p * PO_c + k_so * S(o[c],D2)) + k_pr * (1.0 - (double)o[1-c])
 * G_f and G_p are those of the *_grad entries, with smooth_second_order those of the *_grad_ft entries.  The range is not checked
 * for usability: on a zero or non-finite span the values follow IEEE (NaN or Inf in the elements that read them), which is what the
 * Lua gives; a pixel-direction outside the image is +0.0 / 1.0 whatever the range.  Five places where this is not the derivative of
 * the records' value, all kept:
 *   1. Centre tap only: dl and dcs are the derivative of the pixel's own window term with respect to the pixel's own value; the eight
 *      neighbouring windows that also contain the pixel are dropped.
 *   2. Border: under replication padding a border pixel occurs several times in its own window (a corner pixel has the weight
 *      (gc + ge)^2); the Lua uses gw everywhere.
 *   3. Range: the gradient is with respect to the normalised image; the factor 1 / (mx - mn) and the dependence of mn and mx on the
 *      inputs are absent.
 *   4. Outside the image: a pixel-direction whose target leaves the image adds penalty_out = 1 to the occlusion gradient.
 *   5. Occlusion prior: its 1 - o[other] comes along unchanged.                                                                  */
typedef struct b2f_loss_grad_ssim_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;   /* as b2f_loss_grad_opts */
    double level_weights[7];
    int size_average;
    int smooth_second_order;                                     /* -smooth_second_order: 0 | 1 (orthogonal in model.lua) */
    double ssim_alpha;                                           /* finite, in [0, 1]: 1 is OSSIM, 0.85 OSSIML1 */
} b2f_loss_grad_ssim_opts;
/* b2f_loss_grad_defaults, smooth_second_order = 0, ssim_alpha = 0.85 */
B2F_API int b2f_loss_grad_ssim_defaults(b2f_loss_grad_ssim_opts *opts);
/* The six *_grad_ft entries with these options and the range of the *_ssim entries: the checks of both families (and ssim_alpha in
 * [0, 1]), same sub-batching, same workspaces; a refusal writes nothing.  B2F_SSIM_RANGE_BATCH is refused by the forward entries when
 * the request would be cut into more than one sub-batch, and by the multi entry always.  The optional records of the forward entries
 * are the 32 words of b2f_forward_loss_ssim, from the same pyramid and the same ranges.                                            */
B2F_API int b2f_table_loss_grad_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                  double flow_scale, const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode,
                                  const float *ranges);
B2F_API int b2f_table_loss_grad_ssim_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                    const float *dev_ref, double flow_scale, const b2f_loss_grad_ssim_opts *opts,
                                    float *const *dev_grad, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_op_table_loss_grad_ssim(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                                double flow_scale, const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode,
                                const float *ranges);
B2F_API int b2f_forward_loss_grad_ssim(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                               const b2f_loss_grad_ssim_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                               float *const *outs, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_grad_ssim_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                      const b2f_loss_grad_ssim_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                      int n_outs, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_multi_forward_loss_grad_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                     const b2f_loss_grad_ssim_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                     int range_mode, const float *ranges);
/* ---- the photometric terms without occlusion masking: -pme_criterion BCC | SSIM | SSIML1, and -no_occ (b2f_version() >= 1013) ----
 * opts.lua:62,85, model.lua:149-159: criterions/MBCCriterion.lua and criterions/MSSIML1Criterion.lua, the paper's baseline without
 * occlusion reasoning.  The *_plain entries return records of 40 words per image and level: words 0 .. 15 are those of
 * b2f_table_loss*, bit for bit; words 16 .. 29 the sums below; words 30 .. 39 are 0.  Inputs, R_j, the target coordinate, its inside
 * test and the level scale are those of words 6 .. 9 (MBCCriterion.lua:70-87 and MSSIML1Criterion.lua:120-138 state the test as
 * OBCCriterion.lua:78-100 does); fp64 without fused multiply-adds, the same P1, D1, q, window G, ge, gc, C1, C2 and t(v) as above.
 * A pixel-direction whose target leaves the image contributes nothing, in value and in gradient: there is no penalty_out.
 *   BCC (MBCCriterion.lua:35-102), per direction d and channel c on the raw planes: delta_c = iw_d[c] - R_j[c],
 *     B1 = (P1(delta_0) + P1(delta_1)) + P1(delta_2)     (-pme_penalty L1, model.lua:189-190)
 *     B2 = (delta_0^2 + delta_1^2) + delta_2^2           (the criterion's own QuadraticPenalty; -pme_penalty Quadratic)
 *   SSIM / SSIML1 (MSSIML1Criterion.lua:45-153), on the range-normalised planes x = t(iw_d[c]), y = t(R_j[c]):
 *     S = sum over c of (1.0 - l * cs), B = sum over c of P1(x_c - y_c), as for the *_ssim entries but without the factor o[1 - d]
 *   range: MSSIML1Criterion.lua:63-68 runs `for i = 2,#input` and not from warp_start, so (mn, mx) cover R_j, iw1, iw3, AND the two
 *     occlusion planes, and on Soft tables the two planes of the past flow.  The quirk is kept: the own range of words 28 / 29 is taken
 *     over those planes.  range_mode and ranges as for the *_ssim entries, with the same refusals.
 * A pixel-direction that counts in PHOTO_INSIDE adds q(B1) to PLAIN_L1_Q30[d] and q(B2) to PLAIN_SQ_Q30[d] (q saturates at 16), and,
 * on a usable range and with S and B not NaN, q(S) to PLAIN_SSIM_Q30[d] and q(B) to PLAIN_L1N_Q30[d]; otherwise it adds to neither of
 * these two and counts in PLAIN_SSIM_NONFINITE[d].  The criterion's value at a level is
 *   BCC:            sum over d of PLAIN_L1_Q30[d] (or PLAIN_SQ_Q30[d]) / 2^30 / (3 * 2)
 *   SSIM / SSIML1:  sum over d of (alpha * PLAIN_SSIM_Q30[d] + (1 - alpha) * PLAIN_L1N_Q30[d]) / 2^30 / (3 * 2), alpha = 1 / 0.85
 * times 1 / (h w) under size_average (back2future.loss_summary, which with no_occ drops the occlusions' smoothness and prior as
 * train.lua:456 and test.lua:289 do).                                                                                          */
B2F_API int b2f_table_loss_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                              double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
B2F_API int b2f_table_loss_plain_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                                double flow_scale, unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_op_table_loss_plain(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                            double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_plain(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                           float **outs, int n_outs, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_plain_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                  unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_multi_forward_loss_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                                 int range_mode, const float *ranges);
#define B2F_LOSS_PLAIN_L1_Q30 16           /* [2] sum over PHOTO_INSIDE of q(B1), past / future, 2^-30 */
#define B2F_LOSS_PLAIN_SQ_Q30 18           /* [2] of q(B2) */
#define B2F_LOSS_PLAIN_SSIM_Q30 20         /* [2] of q(S) */
#define B2F_LOSS_PLAIN_L1N_Q30 22          /* [2] of q(B) */
#define B2F_LOSS_PLAIN_SSIM_NONFINITE 24   /* [2] pixel-directions of PHOTO_INSIDE with a NaN S or B or an unusable range */
#define B2F_LOSS_PLAIN_RANGE_USED 26       /* [2] float bits, zero-extended, of the mn / mx used for this image and level */
#define B2F_LOSS_PLAIN_RANGE_OWN 28        /* [2] float bits of this image's own minimum / maximum at this level, occlusions included */
#define B2F_LOSS_PLAIN_WORDS 40            /* words 30 .. 39 are reserved, always 0 */
/* The gradient with respect to the output table (MBCCriterion.lua:104-186, MSSIML1Criterion.lua:155-261, combined with the other
 * criteria as train.lua:428-468 does; -no_occ: smooth_occ = prior_occ = 0).  Everything not named is as for the *_grad_ssim entries.
 *   BCC:   G_iw_d[c] = m_d ? k_p * D1(delta_c) : +0.0    (penalty L1)       or    m_d ? k_p * (2.0 * delta_c) : +0.0    (QUADRATIC)
 *   SSIM:  G_iw_d[c] = m_d ? k_p * T_c : +0.0, T_c as for the *_grad_ssim entries: quirks 1 - 3 there (centre tap only, gw = gc^2 on
 *          the border, no 1 / (mx - mn)) hold here too; a term whose weight is exactly 0 is not evaluated
 *   G_o[c] = k_so * S(o[c],D2) + k_pr * (1.0 - (double)o[1-c]): the photometric criterion gives the occlusions exactly zero
 *          (gradInput[1]:fill(0)); with both weights 0 the planes are +0.0
 *   G_f, G_p: the photometric criteria do not reach the flows; those of the *_grad entries, with smooth_second_order of *_grad_ft.   */
#define B2F_PLAIN_BCC 0
#define B2F_PLAIN_SSIM 1
#define B2F_PLAIN_L1 0
#define B2F_PLAIN_QUADRATIC 1
typedef struct b2f_loss_grad_plain_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;   /* as b2f_loss_grad_opts */
    double level_weights[7];
    int size_average;
    int smooth_second_order;                                     /* -smooth_second_order: 0 | 1 */
    int criterion;                                               /* B2F_PLAIN_BCC | B2F_PLAIN_SSIM */
    int penalty;                                                 /* B2F_PLAIN_L1 | B2F_PLAIN_QUADRATIC; QUADRATIC with BCC only */
    double ssim_alpha;                                           /* finite, in [0, 1]: 1 is SSIM, 0.85 SSIML1; read with B2F_PLAIN_SSIM */
} b2f_loss_grad_plain_opts;
/* b2f_loss_grad_defaults, smooth_second_order = 0, criterion BCC, penalty L1, ssim_alpha = 0.85 */
B2F_API int b2f_loss_grad_plain_defaults(b2f_loss_grad_plain_opts *opts);
/* The six *_grad_ssim entries with these options: their checks and refusals, plus a bad criterion or penalty and, where there is a
 * context, a two_frame model; a refusal writes nothing and launches nothing.  The optional records of the forward entries are the 40
 * words of b2f_forward_loss_plain.  With B2F_PLAIN_BCC the range is still checked and, where records are asked for, computed.     */
B2F_API int b2f_table_loss_grad_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                   double flow_scale, const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode,
                                   const float *ranges);
B2F_API int b2f_table_loss_grad_plain_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                     const float *dev_ref, double flow_scale, const b2f_loss_grad_plain_opts *opts,
                                     float *const *dev_grad, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_op_table_loss_grad_plain(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                                 double flow_scale, const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode,
                                 const float *ranges);
B2F_API int b2f_forward_loss_grad_plain(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                                const b2f_loss_grad_plain_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                float *const *outs, int range_mode, const float *ranges);
B2F_API int b2f_forward_loss_grad_plain_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                       const b2f_loss_grad_plain_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                       int n_outs, void *stream, int range_mode, const float *ranges);
B2F_API int b2f_multi_forward_loss_grad_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                      const b2f_loss_grad_plain_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                      int range_mode, const float *ranges);
/* ---- the supervised objective: -optimize epe (opts.lua:56; b2f_version() >= 1012) ----
 * The supervised branch of train.lua:295-335 at the output table: the masked end-point error of the future flow of every level against
 * ground truth (criterion = nn.L2Criterion, model.lua:145-146,249-251; criterions/L2Criterion.lua:27-71) as integer records per image
 * and level, and its `gradOutputs`.  Inputs beside the table, with the conventions of b2f_flow_score: gt_flow float n x 2 x H x W, the
 * true flow in pixels at the size of level 0; valid uint8 n x H x W or NULL (all valid); gt_occ uint8 n x H x W or NULL, its bytes
 * 0 / 1 / 2 the reference's labels 0 / 0.5 / 1 and anything else unlabelled; rescale = the context's rescale_flow.  Level j reads
 * the full-resolution planes at S = (y << j, x << j): train.lua:298-299 sub-samples with SpatialAveragePooling(1,1,2,2), every second
 * pixel and no averaging.  Per-pixel arithmetic is fp64 without fused multiply-adds, + - * / and sqrt only:
 *   flow (train.lua:312-314):  g_c = ((double)gt_flow[c][S] / flow_scale) / (rescale ? 2^j : 1)   (train.lua:300-302)
 *     d_c = (double)f_c - g_c, e = sqrt(d_0 * d_0 + d_1 * d_1)                                     (L2Criterion.lua:36-37)
 *     valid[S] == 0: nothing is added whatever the values, the gradient is +0.0 (b2f_flow_score's rule; the Lua has NaN * 0 here)
 *     valid, e not finite: FLOW_NONFINITE += 1; valid and finite: VALID += 1, EPE_Q20 += (uint64)(min(e, 65536) * 2^20 + 0.5)
 *     gradient of f_c = (k_j * d_c) / (e + 1e-12), also where e is not finite                      (L2Criterion.lua:58-64)
 *   occlusions (train.lua:316-332, opt-in: evaluated only when occ > 0, else words 4 .. 6 are 0 and the planes +0.0).  The Lua as written
 *     cannot run (it slices the labels to one channel, then indexes channel 2, and hands L2Criterion a tensor for {target, mask}); its
 *     intent, consistent with train.lua:387: t_0 = [g == 0] + 0.5 [g == 0.5], t_1 = [g == 1] + 0.5 [g == 0.5], on labelled pixels
 *     whatever `valid` says: q = sqrt((o_0 - t_0)^2 + (o_1 - t_1)^2); LABELLED, OCC_Q20, OCC_NONFINITE as above; gradient of
 *     o_c = (k'_j * (o_c - t_c)) / (q + 1e-12); unlabelled pixels add nothing and get +0.0
 *   k_j = epe * lw_j, k'_j = occ * lw_j (train.lua:328,331 give the occlusion term no option weight); with size_average lw_j = 1
 *     (train.lua:60-64) and k_j = epe / N_j, k'_j = occ / N'_j, N_j / N'_j the valid / labelled source pixels of level j (mask:sum(),
 *     L2Criterion.lua:34,56) by count_mode: B2F_EPE_COUNT_BATCH over the n images of the call (the reference's), B2F_EPE_COUNT_IMAGE each
 *     image's own, B2F_EPE_COUNT_GIVEN counts[2 j] / counts[2 j + 1] (a host array of L x 2 doubles, NULL in the other modes).  A
 *     factor of exactly 0 -- a weight of 0, or no counted pixel, where the Lua divides by zero -- gives +0.0, not evaluated.
 *   Every gradient element is formed in fp64 and rounded to fp32 once, on store.  The gradient table has the shapes of the table; the
 *   future flow and, with occ > 0, the occlusions are as above, every other tensor is +0.0.
 * loss: n x L records of B2F_LOSS_EPE_WORDS words, image-major; integer sums, so a record does not depend on the grid or on where a
 * request is cut.  The reported epe of train.lua:340-344 is flow_scale * sum EPE_Q20[level 0] / 2^20 / sum VALID[level 0]
 * (back2future.loss_summary(objective="epe")).  test.lua:150-180 (three arguments to criterion:forward, a 2 x 2 mean of the flow) is
 * not followed.  Checks: those of b2f_table_loss*; in addition a null gt_flow, negative or non-finite weights or counts, occ > 0
 * without gt_occ, a bad count_mode, loss and grad both NULL, and an output that aliases an input are refused with nothing written. */
#define B2F_LOSS_EPE_PIXELS 0          /* h * w of the level */
#define B2F_LOSS_EPE_VALID 1           /* valid pixels with a finite error */
#define B2F_LOSS_EPE_Q20 2             /* their end-point error in units of flow_scale pixels, 2^-20 */
#define B2F_LOSS_EPE_FLOW_NONFINITE 3  /* valid pixels with a non-finite error */
#define B2F_LOSS_EPE_LABELLED 4        /* labelled pixels with a finite occlusion error (0 unless occ > 0) */
#define B2F_LOSS_EPE_OCC_Q20 5         /* their occlusion error, 2^-20 */
#define B2F_LOSS_EPE_OCC_NONFINITE 6   /* labelled pixels with a non-finite occlusion error */
#define B2F_LOSS_EPE_WORDS 8           /* word 7 is reserved, always 0 */
#define B2F_EPE_COUNT_BATCH 0          /* count_mode: N_j, N'_j over the n images of the call */
#define B2F_EPE_COUNT_IMAGE 1          /* each image's own */
#define B2F_EPE_COUNT_GIVEN 2          /* counts[2 j], counts[2 j + 1] */
typedef struct b2f_loss_epe_opts {
    double epe;                /* -epe, opts.lua: the weight of the flow term */
    double occ;                /* the weight of the occlusion term; 0 (the default) leaves it out */
    int size_average;          /* -sizeAverage */
    double level_weights[7];   /* train.lua:56-58; not read with size_average */
} b2f_loss_epe_opts;
/* epe = 1, occ = 0, size_average = 0, the level weights of train.lua:56-58 */
B2F_API int b2f_loss_epe_defaults(b2f_loss_epe_opts *opts);
/* host only, no GPU: train.lua:296-334 per pixel on the CPU.  table as for b2f_table_loss_host; loss (n x L x 8 words) and grad (the
 * table's n_outs tensors) may each be NULL, not both; opts NULL: the defaults.                                                      */
B2F_API int b2f_table_loss_epe_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *gt_flow,
                            const unsigned char *valid, const unsigned char *gt_occ, double flow_scale, int rescale,
                            const b2f_loss_epe_opts *opts, int count_mode, const double *counts, unsigned long long *loss,
                            float *const *grad);
/* train.lua:296-334 on device pointers (L2Criterion.lua:27-71 per pixel): dev_table and dev_grad are host arrays of n_outs device
 * pointers, 16-byte aligned like dev_gt_flow and dev_loss; dev_valid and dev_gt_occ need no alignment.  Asynchronous on `stream`;
 * dev_loss is zeroed on the stream first.  With size_average and a gradient table, a counting pass over dev_valid / dev_gt_occ runs
 * first, into a workspace of the context: calls on different streams must be ordered by the caller.  At most 65535 images per call. */
B2F_API int b2f_table_loss_epe_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                              const float *dev_gt_flow, const unsigned char *dev_valid, const unsigned char *dev_gt_occ,
                              double flow_scale, const b2f_loss_epe_opts *opts, int count_mode, const double *counts,
                              unsigned long long *dev_loss, float *const *dev_grad, void *stream);
/* train.lua:296-334 on host pointers through the GPU, like b2f_op_table_loss */
B2F_API int b2f_op_table_loss_epe(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *gt_flow,
                          const unsigned char *valid, const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts,
                          int count_mode, const double *counts, unsigned long long *loss, float *const *grad);
/* model:forward followed by train.lua:296-334 without the download of the table: x as for b2f_forward_loss; gt_flow / valid / gt_occ of
 * the n triplets in host memory, uploaded with the frames of each sub-batch (host_subbatch_pixels); loss (n x L x 8 words), grad (the
 * table's n_outs tensors) and outs (the table itself, n_outs tensors) may each be NULL, loss and grad not both.  B2F_EPE_COUNT_BATCH
 * counts over the caller's whole n before the first sub-batch, so a cut changes nothing.  two_frame is refused.                   */
B2F_API int b2f_forward_loss_epe(b2f_ctx *ctx, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                         const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode,
                         const double *counts, unsigned long long *loss, float *const *grad, int n_outs, float *const *outs);
/* the same on device pointers (dev_in as for b2f_forward_loss_device, B2F_IN_NORMALIZED only); asynchronous on `stream`; with a
 * gradient table and size_average, B2F_EPE_COUNT_BATCH is refused when the request would be cut into more than one sub-batch      */
B2F_API int b2f_forward_loss_epe_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, const float *dev_gt_flow,
                                const unsigned char *dev_valid, const unsigned char *dev_gt_occ, double flow_scale,
                                const b2f_loss_epe_opts *opts, int count_mode, const double *counts, unsigned long long *dev_loss,
                                float *const *dev_grad, int n_outs, void *stream);
/* ... over several GPUs: the n triplets and their ground truth are split with b2f_shard_range; B2F_EPE_COUNT_BATCH is refused (a
 * shard's counts would depend on the split); one context's words and bits                                                        */
B2F_API int b2f_multi_forward_loss_epe(b2f_multi *m, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                               const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode,
                               const double *counts, unsigned long long *loss, float *const *grad, int n_outs);
/* ---- streams: frames that arrive one at a time (a camera, a decoder, a ROS node) ----
 * back2future.lua:47-95 takes three whole frames per call, so a live caller of the reference hands every
 * frame to computeFlow three times (as im3, then im2, then im1) and pays three uploads and three feature
 * pyramids for it.  A stream keeps the pyramid features of the last frames on the GPU: every pushed frame is
 * uploaded once and goes through the pyramid (pwc.lua:169-211) once.  It serves `cams` cameras that deliver
 * their frames in lockstep (1: one camera, 2: a stereo rig, ...).  Pushes are numbered k = 1, 2, 3, ... since
 * open / the last reset: pushes 1 and 2 set *ready = 0 and write nothing; push k >= 3 sets *ready = 1 and
 * writes, per camera, the outputs of the triplet of frames (k-2, k-1, k) -- the flow of centre frame k-1.
 * With the context's default options these are output k-3 of b2f_compute_flow_sequence_f32 on the same
 * frames (T >= 4) bit for bit: a stream follows the kernel rule of a batch whatever `cams` is; with option
 * adaptive_kernels = 1 it follows the per-launch rule (the flow is then within 1e-3 of the default one).
 *
 * b2f_stream_open replaces the `model` global's implicit state (back2future.lua:113) for this pattern: cams >= 1,
 * in_kind = B2F_IN_UNIT (floats in [0,1]) or B2F_IN_U8 (bytes, value = byte / 255), H0, W0 >= 64 (any size:
 * frames are rescaled to multiples of 64 as in :54-71).  The stream owns one device block (three slots of
 * features and frames per camera: about 3 x 28 MB per camera at 1024 x 1920, plus the frames and the
 * buffers of a push) that no other call on the context touches; the shipped graph only (a context made with
 * b2f_init_ex options is refused).  The context owns its streams: b2f_destroy closes those still open.   */
typedef struct b2f_stream b2f_stream;
B2F_API int b2f_stream_open(b2f_ctx *ctx, int cams, int in_kind, int H0, int W0, b2f_stream **out);
/* Waits for the stream's work, frees its memory and drops the context's captured graphs (they hold its
 * pointers).  NULL is a no-op.                                                                         */
B2F_API void b2f_stream_close(b2f_stream *st);
/* Forgets the pushed frames (the next push is push 1 again) and clears the broken flag a failed push sets. */
B2F_API int b2f_stream_reset(b2f_stream *st);
/* cams, H0, W0, in_kind and the frames pushed since open / the last reset (any pointer may be NULL). */
B2F_API int b2f_stream_info(const b2f_stream *st, int *cams, int *H0, int *W0, int *in_kind, long long *pushed);
/* One new frame per camera from host memory, replacing one computeFlow(im1, im2, im3) call
 * (back2future.lua:47-95) per new frame.
 * frames: cams x 3 x H0 x W0 floats or bytes (the stream's in_kind); outputs as b2f_compute_flow_batch_f32
 * with n = cams: flow cams x 2 x H0 x W0 floats (required), occ_prob cams x 2 x H0 x W0 floats,
 * fwd_occ / bwd_occ cams x H0 x W0 bytes (NULL: neither computed nor downloaded).  Synchronous: one upload of
 * the cams frames (bytes as bytes; page-locked memory is DMA'd in place, pageable memory goes through the
 * stream's staging block), the kernels, the download of what was asked for.  A malformed push (NULL required
 * pointer, device memory) fails before any HIP work and leaves the stream as it was; a HIP failure inside a
 * push marks the stream broken: later pushes fail, saying so, until b2f_stream_reset.                  */
B2F_API int b2f_stream_push(b2f_stream *st, const void *frames, float *flow, float *occ_prob,
                    unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready);
/* The same with flow pictures as the output, as b2f_compute_flow_batch_rgb with n = cams: rgb is required,
 * max_used, flow and the masks are optional; a live preview downloads 3 bytes per pixel.                */
B2F_API int b2f_stream_push_rgb(b2f_stream *st, const void *frames, double max_norm, int layout, unsigned char *rgb,
                        double *max_used, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready);
/* The same on GPU memory, asynchronous on `stream` like b2f_compute_flow_device (frames decoded on the GPU):
 * every pointer device memory and 16-byte aligned; dev_frames is read before the call returns control to
 * `stream`'s next work, so the caller may overwrite it after anything ordered behind the push.  Pushes of one
 * stream must be ordered by the caller (one hipStream, or events).  Pictures on the device: b2f_flow_rgb_device
 * on dev_flow, on the same stream.  *ready is known when the call returns.                               */
B2F_API int b2f_stream_push_device(b2f_stream *st, const void *dev_frames, float *dev_flow, float *dev_occ_prob,
                           unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream, int *ready);
/* ---- streams with motion compensation and the past flow per pushed frame ----
 * b2f_stream_open_ex is b2f_stream_open with `flags`, a sum of B2F_STREAM_*; flags = 0 is b2f_stream_open itself, with the
 * same device block.  What a flag adds is kept for the stream's lifetime:
 *   B2F_STREAM_WARP  the stream keeps the caller's own frames of its last three pushes, which the warp of
 *                    models/pwc.lua:67-73 samples at H0 x W0: at a /64 size its frame slots hold them already, at any
 *                    other size (where those hold the normalized, rescaled frames of back2future.lua:54-71) a ring of
 *                    3 slots x cams frames as pushed, 3 x H0 x W0 bytes or floats per camera and slot.  Every push of
 *                    such a stream, of whichever entry, keeps its frames, so plain and warp pushes may alternate.  It
 *                    also holds the warped frames and the photometric records of a host push.
 *   B2F_STREAM_PAST  the stream may run the past-flow decoders (models/pwc.lua:328-385) and holds the past flow of a
 *                    push; refused, in the words of the _past entries, on a context without them.
 * b2f_stream_flags returns the flags a stream was opened with.                                                        */
enum { B2F_STREAM_WARP = 1, B2F_STREAM_PAST = 2 };
B2F_API int b2f_stream_open_ex(b2f_ctx *ctx, int cams, int in_kind, int H0, int W0, int flags, b2f_stream **out);
B2F_API int b2f_stream_flags(const b2f_stream *st, int *flags);
/* b2f_compute_flow_sequence_warp (own_past = 0) and b2f_compute_flow_sequence_warp_past (own_past != 0) for one new frame
 * per camera: from the third push on the outputs of the triplet (k-2, k-1, k) -- the frames of pushes k-2 and k
 * warped onto the frame of push k-1 (test.lua:285's inputs, models/pwc.lua:67-73) and the photometric record
 * (criterions/OBCCriterion.lua:79-100) -- which are output k-3 of that sequence entry on the same frames, bit for bit.
 * warped: cams x 2 x 3 x H0 x W0 in the stream's element type; photo: cams x B2F_PHOTO_WORDS words; at least one of
 * the two is required, every other output is optional (NULL: neither computed nor downloaded).  past_flow: the past
 * flow as in the _past entries; it and own_past need B2F_STREAM_PAST, the call itself B2F_STREAM_WARP.  A push the
 * stream was not opened for, one with neither warped nor photo, or with a flow_scale that is not finite and > 0
 * fails before any HIP work, names the flag or the argument, and leaves the stream as it was.  A host entry,
 * synchronous like b2f_stream_push.                                                                              */
B2F_API int b2f_stream_push_warp(b2f_stream *st, const void *frames, double flow_scale, int own_past, void *warped,
                         unsigned long long *photo, float *flow, float *occ_prob, unsigned char *fwd_occ,
                         unsigned char *bwd_occ, float *past_flow, int *ready);
/* The same on GPU memory, asynchronous on `stream` like b2f_stream_push_device (every pointer device memory, 16-byte
 * aligned); dev_frames is copied into the stream before the call returns control to `stream`'s next work.          */
B2F_API int b2f_stream_push_warp_device(b2f_stream *st, const void *dev_frames, double flow_scale, int own_past, void *dev_warped,
                                unsigned long long *dev_photo, float *dev_flow, float *dev_occ_prob,
                                unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, float *dev_past_flow, void *stream,
                                int *ready);
/* b2f_compute_flow_sequence_past / b2f_compute_flow_sequence_device_past for one new frame per camera: b2f_stream_push
 * and b2f_stream_push_device with the past flow (skip_ubfs[3], models/pwc.lua:328-385) behind the flow; needs
 * B2F_STREAM_PAST.  A NULL past_flow makes it the plain push.                                                     */
B2F_API int b2f_stream_push_past(b2f_stream *st, const void *frames, float *flow, float *past_flow, float *occ_prob,
                         unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready);
B2F_API int b2f_stream_push_past_device(b2f_stream *st, const void *dev_frames, float *dev_flow, float *dev_past_flow,
                                float *dev_occ_prob, unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream,
                                int *ready);
/* Full output table of model:forward (pwc.lua:459-489) into n_outs host buffers, in
 * table order; x is B x 9 x H x W normalized host memory.                           */
B2F_API int b2f_forward(b2f_ctx *ctx, const float *x, int B, int H, int W, float **outs, int n_outs);
B2F_API int b2f_output_shapes(const b2f_ctx *ctx, int H, int W, int *ch, int *oh, int *ow, int cap);

/* Execution options: use_graph (default 0) = b2f_forward_device replays a hipGraph per
 * (shape, pointers) combination, captured on its second use; host_graph (default 1) = the
 * same inside b2f_compute_flow*; profile = record HIP events around every kernel launch
 * (eager mode); profile_layers = one profile row per layer shape.
 * Kernel selection: wino4_min_pixels (default 4096) = stride-1 convs run the Winograd F(4x4)
 * kernel on maps of at least that many pixels and F(2x2) below -- a rule of the map size only,
 * so a triplet's result never depends on the batch it is computed in; wino_split_pixels (default
 * 512) = F(2x2) launches on maps of at most that many pixels run one block per 32 outputs
 * (twice the blocks for the coarsest level; same bits); adaptive_kernels = 1
 * picks the variant per launch by block rounds on the 256 CUs instead (faster for single
 * triplets, results then vary at the 1e-6 level with the batch size); corr_variant (-1 auto /
 * 0 .. 7) forces an instantiation of the warp + cost-volume kernel (same bits either way);
 * wino4_persistent (default 1) = F(4x4) launches run as persistent blocks, one per CU
 * (0: one tile per block; same bits either way); s2_tiles_per_block
 * (default 0 = launcher's rule) = tiles a block of the stride-2 kernel chains (same bits);
 * wino8 / s2_tile_groups (default 1) = launches that cannot fill the chip (a single triplet's
 * coarse levels) run the eight-wave F(2x2) kernel / one 32-output tile per stride-2 block
 * (more, lighter blocks; same bits).
 * Host pipeline of b2f_compute_flow*: host_subbatch_pixels, host_threads (0 = auto), host_u8,
 * host_ramp.  The library reads no environment variable after b2f_init (which takes
 * B2F_<OPTION> as the initial value of the tuning options).                              */
B2F_API int b2f_set_option(b2f_ctx *ctx, const char *key, int value);
B2F_API int b2f_get_option(const b2f_ctx *ctx, const char *key, int *value);
/* Per-kernel-class timings gathered while profile=1.  names: cap x 32 chars.  A context keeps
 * every row name it has used; *n = min(cap, rows): *n == cap means that rows may have been
 * left out, *n < cap that these are all (call again with a larger cap).               */
B2F_API int b2f_profile_read(b2f_ctx *ctx, char *names, double *total_ms, long long *launches,
                     int cap, int *n);
B2F_API int b2f_profile_reset(b2f_ctx *ctx);
B2F_API int b2f_synchronize(b2f_ctx *ctx);

/* ---- op-level entry points (host pointers, layouts of the reference modules) ----
 * nn.CostVolMulti(win, fwd):updateOutput({ref, frm}) -- models/CostVolMulti.lua:49-109;
 * ref, frm: B x C x h x w; out: B x win*win x h x w.                               */
B2F_API int b2f_op_costvol(b2f_ctx *ctx, const float *ref, const float *frm, int B, int C, int h,
                   int w, int win, int fwd, float *out);
/* nn.BilinearSamplerBHWD:updateOutput({img, grid}), CUDA semantics --
 * extras/stnbhwd/BilinearSamplerBHWD.cu:41-158; img: B x ih x iw x C, grid:
 * B x gh x gw x 2 (x first), out: B x gh x gw x C.                                  */
B2F_API int b2f_op_warp_bhwd(b2f_ctx *ctx, const float *img, const float *grid, int B, int ih,
                     int iw, int C, int gh, int gw, float *out);
/* Backward passes of the two custom modules (training side; not used by computeFlow).
 * nn.BilinearSamplerBHWD:updateGradInput -- BilinearSamplerBHWD.lua:81-107, CUDA kernel
 * BilinearSamplerBHWD.cu:161-307: grad_out B x gh x gw x C -> grad_img B x ih x iw x C (zeroed, then
 * accumulated; NULL = the onlyGrid instantiation, :372-421) and grad_grid B x gh x gw x 2 (x first).      */
B2F_API int b2f_op_warp_bhwd_backward(b2f_ctx *ctx, const float *img, const float *grid,
                              const float *grad_out, int B, int ih, int iw, int C, int gh, int gw,
                              float *grad_img, float *grad_grid);
/* nn.CostVolMulti(win, fwd):updateGradInput({ref, frm}, grad_out) -- models/CostVolMulti.lua:111-181:
 * grad_out B x win*win x h x w -> grad_ref, grad_frm B x C x h x w.                                       */
B2F_API int b2f_op_costvol_backward(b2f_ctx *ctx, const float *ref, const float *frm,
                            const float *grad_out, int B, int C, int h, int w, int win, int fwd,
                            float *grad_ref, float *grad_frm);
/* The fused kernel the pipeline uses for pwc.lua:246-267 + :393-409: warp both
 * neighbour maps by +k*flow (future) / -k*flow (past) and emit the joined
 * 162-channel cost volume.  ref/nbr_future/nbr_past: B x C x h x w; flow: B x 2 x h x w
 * or NULL (level 7: no warp); out: B x 162 x h x w.                                 */
B2F_API int b2f_op_warp_costvol(b2f_ctx *ctx, const float *ref, const float *nbr_future,
                        const float *nbr_past, const float *flow, float k, int B, int C,
                        int h, int w, float *out);
/* nn.SpatialConvolution(Ci,Co,3,3,s,s,1,1) [+ nn.LeakyReLU(0.2)] -- pwc.lua:58-85;
 * x: B x Ci x H x W, w: Co x Ci x 3 x 3, y: B x Co x Ho x Wo.                       */
B2F_API int b2f_op_conv3x3(b2f_ctx *ctx, const float *x, int B, int Ci, int H, int W, const float *w,
                   const float *bias, int Co, int stride, int leaky, float *y);
/* nn.SpatialConvolution(Ci,Co,3,3,1,1,1,1) [+ LeakyReLU(0.2)] :backward -- x: B x Ci x H x W, w: Co x Ci x 3 x 3,
 * y: the layer's output (read only when leaky; NULL otherwise), grad_y: B x Co x H x W.  Any of grad_x (B x Ci x H x W),
 * grad_w (Co x Ci x 3 x 3), grad_b (Co) may be NULL: not computed.  layout 0: NHWC strides on the device (as b2f_op_conv3x3),
 * 1: the forward's chunk-planar strides.  stride != 1 is refused.  Host pointers, planar.
 * g' = grad_y * (y > 0 ? 1 : 0.2f) with leaky (y == 0 takes the slope), else grad_y; grad_x = conv3x3(g', w rotated by 180 degrees and
 * channel-transposed) on the forward's own kernels (the profile row is the forward kernel's); grad_w[co][ci][ky][kx] = sum over
 * (b, oy, ox) of g'[b][co][oy][ox] * x[b][ci][oy + ky - 1][ox + kx - 1] on the fp32 MFMA and grad_b[co] = sum of g'[b][co], both as
 * partial sums over disjoint pixel ranges that are added in index order: no atomics, the same bits on any device and in any run.
 * grad_w and grad_b are written, not accumulated.  Refused, with b2f_last_error naming the argument and nothing written: NULL x, w or
 * grad_y; leaky without y; all three outputs NULL; stride != 1; a layout other than 0 / 1; non-positive sizes (b2f_version() >= 1014). */
B2F_API int b2f_op_conv3x3_backward(b2f_ctx *ctx, const float *x, int B, int Ci, int H, int W, const float *w, int Co,
                                    int stride, int leaky, const float *y, const float *grad_y, int layout,
                                    float *grad_x, float *grad_w, float *grad_b);
/* What a b2f_op_conv3x3_backward call of these sizes does to grad_w and grad_b under the context's options: the number of partial sums
 * (a function of B, Ci, H, W, Co alone unless option op_gradw_partials > 0 forces it) and the most pixels one partial sum adds up.
 * Either pointer may be NULL.  Makes no HIP call.                                                                                */
B2F_API int b2f_op_conv3x3_backward_plan(b2f_ctx *ctx, int B, int Ci, int H, int W, int Co, int *partials, long long *longest_chain);
/* nn.SpatialConvolution(Ci,Co,3,3,2,2,1,1) [+ LeakyReLU(0.2)] :backward -- pwc.lua:58-65, the first conv of a convUnit.  x: B x Ci x H x W
 * (H, W: the INPUT map), w: Co x Ci x 3 x 3, y (read only when leaky) and grad_y: B x Co x Ho x Wo, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.
 * Outputs, layout, g', the partial sums of grad_w / grad_b and the refusals are b2f_op_conv3x3_backward's (there is no stride argument).
 * grad_x[b][ci][iy][ix] = sum over (co, ky, kx) with iy + 1 - ky and ix + 1 - kx even and inside 2 Ho x 2 Wo of
 * g'[b][co][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2] * w[co][ci][ky][kx]: a transposed convolution on a kernel of its own (profile row
 * convbwd_gradx_s2) that multiplies the nine taps a 2 x 2 block of input pixels has; grad_w[co][ci][ky][kx] = sum over (b, oy, ox) of
 * g'[b][co][oy][ox] * x[b][ci][2 oy + ky - 1][2 ox + kx - 1], zero outside the map (b2f_version() >= 1015).                            */
B2F_API int b2f_op_conv3x3s2_backward(b2f_ctx *ctx, const float *x, int B, int Ci, int H, int W, const float *w, int Co,
                                      int leaky, const float *y, const float *grad_y, int layout,
                                      float *grad_x, float *grad_w, float *grad_b);
/* b2f_op_conv3x3_backward_plan for a b2f_op_conv3x3s2_backward call: H, W are the input map's, the chain counts in-map OUTPUT pixels.
 * Either pointer may be NULL.  Makes no HIP call.                                                                                */
B2F_API int b2f_op_conv3x3s2_backward_plan(b2f_ctx *ctx, int B, int Ci, int H, int W, int Co, int *partials, long long *longest_chain);
/* Two entries that run a piece of the loaded model in the forward pass's own layout (chunk-planar buffers, the context's packed
 * weights and options), for the tests of tests/test_gpu_in_place.py.
 * b2f_op_layer: conv (kind, level, idx) of the context's packed table -- kind 0 feature pyramid (level 2..7, idx 1..2; not feat2.conv1),
 * 1 occlusion / 2 flow / 3 past-flow decoder (level 3..7, idx 1..6) -- through the launch path of the forward, the kernel chosen under the
 * context's options for a batch of nimg.  x: nimg x Ci x H x W in the layer's Torch input order (a first decoder layer:
 * {cv 162, cs[ref] C_l, flow 2}, pwc.lua:308,334,337), y: nimg x Co x Ho x Wo.  The cost-volume record slots the layer does not read
 * hold 1 + op_hole_fill + slot / 256 (option op_hole_fill, default 0): non-zero, finite, and without effect on y.  Shipped graph only. */
B2F_API int b2f_op_layer(b2f_ctx *ctx, int kind, int level, int idx, int nimg, int H, int W, const float *x, float *y);
/* b2f_op_cv_record: the warp + cost-volume kernel on the forward's strides under option corr_variant.  ref / nbr_future / nbr_past:
 * B x C x h x w (C a multiple of 8); flow, flow_b: B x 2 x h x w or NULL; rec: the whole record, B x 168 x h x w in slot order
 * (fwd 0..79 | bwd 0..79 | fwd 80, bwd 80, flow u v, flow_b u v, 0, 0).                                                          */
B2F_API int b2f_op_cv_record(b2f_ctx *ctx, const float *ref, const float *nbr_future, const float *nbr_past, const float *flow,
                     const float *flow_b, float k, int B, int C, int h, int w, float *rec);
/* b2f_op_cv_variant: which instantiation of the warp + cost-volume kernel (0, 1, 3, 5 or 7; the experiments build adds 2, 4, 6, 8) the
 * launcher runs for a B x C x h x w call under the context's options (corr_variant -1: the automatic rule, by map size, launch size, the
 * device's compute-unit count and C), on the strides of b2f_op_warp_costvol (layout 0) or of b2f_op_cv_record (layout 1).  Launches
 * nothing.  Returns the variant, or -1 with b2f_last_error set.                                                                   */
B2F_API int b2f_op_cv_variant(b2f_ctx *ctx, int B, int C, int h, int w, int layout);
/* The two 16-channel layers of the head of the pyramid as the pipeline runs them with option bf16_direct = 2, in one kernel:
 * nn.SpatialConvolution(16,16,3,3,1,1,1,1) + LeakyReLU(0.2) (pwc.lua:62, level-2 convUnit) followed by
 * nn.SpatialConvolution(16,32,3,3,2,2,1,1) + LeakyReLU(0.2) (pwc.lua:60, level-3 convUnit).
 * x: B x 16 x H x W, w1: 16 x 16 x 3 x 3, w2: 32 x 16 x 3 x 3, y: B x 32 x ceil(H/2) x ceil(W/2).                       */
B2F_API int b2f_op_conv_head16(b2f_ctx *ctx, const float *x, int B, int H, int W, const float *w1, const float *b1,
                       const float *w2, const float *b2, float *y);
/* The first conv of the pyramid as the forward launches it: nn.SpatialConvolution(3,16,3,3,2,2,1,1) + LeakyReLU(0.2) (pwc.lua:59) on each
 * of the three frames, after ColorNormalize when normalize != 0.  x: B x 9 x H x W (frame f in planes 3f .. 3f + 2), H and W even;
 * w: 16 x 3 x 3 x 3, b: 16; y: 3B x 16 x H/2 x W/2, image f * B + b.                                                       */
B2F_API int b2f_op_conv_first(b2f_ctx *ctx, const float *x, int B, int H, int W, int normalize, const float *w, const float *b, float *y);
/* nn.SpatialUpSamplingBilinear(2) on a 2-channel flow field -- pwc.lua:360-381;
 * x: B x 2 x h x w -> y: B x 2 x 2h x 2w.                                            */
B2F_API int b2f_op_upsample_flow2x(b2f_ctx *ctx, const float *x, int B, int h, int w, float *y);
/* image.scale(src, Wd, Hd) 'bilinear' [torch/image] as computeFlow uses it -- back2future.lua:71 -- with
 * ColorNormalize (transforms.lua:33-45, plane % 3 = colour) applied first when normalize != 0;
 * src: C x Hs x Ws -> dst: C x Hd x Wd.  Bit-identical to the CPU routine.             */
B2F_API int b2f_op_image_scale(b2f_ctx *ctx, const float *src, int C, int Hs, int Ws, int normalize,
                       float *dst, int Hd, int Wd);

/* ---- the small kernels of a forward pass, one entry per launcher (tests/test_gpu_glue_float64.py; b2f_version() >= 1009) ----
 * Each entry uploads the host arrays as they are, runs ONE launcher with the stride arguments it is given, and downloads the result:
 * nothing is repacked, so the caller lays records out as the forward does (an 8-float record whose slots the kernel does not own may
 * hold NaN).  Outputs start as a NaN pattern: an element the kernel leaves out stays NaN.
 * b2f_op_upsample_flow2x_ex: nn.SpatialUpSamplingBilinear(2) (pwc.lua:360-381) of the first two floats of the ps-float records
 * x: B x h x w x ps (ps even; the forward: 8, and 2 for the second step); planar = 0: y B x 2h x 2w x 2 (launch_upsample_flow2x),
 * planar = 1: y B x 2 x 2h x 2w (launch_upsample_flow2x_planar).  2h > 65535 is an error.                                     */
B2F_API int b2f_op_upsample_flow2x_ex(b2f_ctx *ctx, const float *x, int ps, int B, int h, int w, int planar, float *y);
/* nn.SpatialSoftMax over the first two floats of the ps-float records logits: B x h x w x ps + two nn.SpatialUpSamplingNearest(2)
 * (pwc.lua:308-321) -> out: B x 2 x 4h x 4w.  4h > 65535 is an error.                                                          */
B2F_API int b2f_op_softmax_nearest4(b2f_ctx *ctx, const float *logits, int ps, int B, int h, int w, float *out);
/* nn.SpatialAveragePooling(2,2,2,2) (pwc.lua:155) on x: nimg x H x W x C (C a multiple of 4) -> y: nimg x H/2 x W/2 x C.        */
B2F_API int b2f_op_avgpool2(b2f_ctx *ctx, const float *x, int nimg, int H, int W, int C, float *y);
/* The packed frames of a triplet batch: x B x 9 x H x W -> img 3 x B x H x W x 8 (frame-major; RGB, ColorNormalize when normalize != 0,
 * then five zeros).                                                                                                              */
B2F_API int b2f_op_pack_input(b2f_ctx *ctx, const float *x, int normalize, int B, int H, int W, float *img);
/* The three image warps by k * flow (flow: B x 2 x H x W planar; out: B x 3 x H x W).  which = 0: launch_warp_image_planar, in = B x H x W
 * x 8 packed frames; 1: launch_warp_input_planar, in = B x 9 x H x W, frame 0..2, in_kind B2F_IN_NORMALIZED / B2F_IN_UNIT; 2:
 * launch_warp_input_seq, in = B x 3 x H x W samples of in_kind (B2F_IN_U8: bytes).                                               */
B2F_API int b2f_op_warp_image(b2f_ctx *ctx, int which, const void *in, int in_kind, int frame, const float *flow, float k, int B,
                      int H, int W, float *out);
/* b2f_op_conv_first on the frames of a sequence (launch_conv_first_seq): x T x 3 x H x W samples of in_kind, H and W even;
 * w: 16 x 3 x 3 x 3, b: 16; y: T x 16 x H/2 x W/2.                                                                               */
B2F_API int b2f_op_conv_first_seq(b2f_ctx *ctx, const void *x, int in_kind, int T, int H, int W, const float *w, const float *b, float *y);
/* Layout changes.  which = 0: launch_nhwc_to_planar, in B x h x w x pix_stride -> out B x C x h x w; 1: launch_cp8_to_planar, in
 * B x ceil(C/8) x h x w x 8 -> out B x C x h x w; 2: launch_planar_to_nhwc, in B x C x h x w -> out B x h x w x pix_stride (zeros
 * from channel C on).                                                                                                            */
B2F_API int b2f_op_layout(b2f_ctx *ctx, int which, const float *in, int C, int pix_stride, int B, int h, int w, float *out);
/* The node kernels of the generic executor (csrc/b2f_graph.hip), chunk-planar maps B x chunks x hw x 8.
 * put_channels: C channels of src (kind 0: chunk-planar with src_chunks planes, 1: packed B x hw x C, 2: planar B x C x hw) into
 * channels c_off .. c_off + C - 1 of dst (in and out).
 * costvol: nn.CostVolMulti(win){ref, frmF} joined with (win, false){ref, frmB} (frmB may be NULL) into dstJ (chunksJ planes; what
 * the kernel does not write stays NaN), and their sum into dstS (or NULL).
 * warp: warpingUnit(img, k * flow), flow packed B x hw x 2.  add_flow: fs[pix][0..1] += u[pix][0..1] on 8-float records.
 * scale: p[i] *= k.  softmax_nearest: as b2f_op_softmax_nearest4 with ps = 8 and any factor f.                                   */
B2F_API int b2f_op_graph_put_channels(b2f_ctx *ctx, const float *src, int kind, int src_chunks, int C, int B, int hw, float *dst,
                              int dst_chunks, int c_off);
B2F_API int b2f_op_graph_costvol(b2f_ctx *ctx, const float *ref, const float *frmF, const float *frmB, int chunks, int C, int B, int h,
                         int w, int win, float *dstJ, int chunksJ, float *dstS, int chunksS);
B2F_API int b2f_op_graph_warp(b2f_ctx *ctx, const float *img, int chunks, const float *flow, float k, int B, int h, int w, float *out);
B2F_API int b2f_op_graph_add_flow(b2f_ctx *ctx, float *fs, const float *u, long long npix);
B2F_API int b2f_op_graph_scale(b2f_ctx *ctx, float *p, long long n, float k);
B2F_API int b2f_op_graph_softmax_nearest(b2f_ctx *ctx, const float *logits, int B, int h, int w, int f, float *out);
/* y[i] = expf(x[i]), the library function of the two softmax kernels as their sources compile it: the yardstick of their bound.  */
B2F_API int b2f_op_expf(b2f_ctx *ctx, const float *x, long long n, float *y);


/* ---- guards (tests) ----
 * Options arena_guard (floats, a multiple of 64; default 0) and arena_fill (0 / 1; default 0), b2f_set_option only: the workspace of the
 * forward pass gets arena_guard floats in front of its first buffer and behind every buffer, and starts as the 32-bit pattern 0x7fc0a5a5
 * (a quiet NaN) instead of zero, as does the device block of a stream opened afterwards.  Setting either frees the workspace and drops
 * the captured graphs.  A kernel may read outside its tensors only if the value cannot reach a result, and may write nowhere outside them:
 * under the two options a result that changes, or a guard word that changes, shows a kernel that does not keep to that.  A context made
 * with graph options lays its workspace out buffer by buffer in the same way, each buffer named by role and level ("occ.in[4]"); and with
 * arena_guard set every tensor of b2f_forward's output table is a device buffer with the pattern on both sides and inside until it is
 * written, checked before the download: a changed word fails the call, b2f_last_error naming the tensor ("b2f_forward output occs[4]").
 * b2f_arena_check: synchronises, and returns the number of guard words of the last pass's layout that no longer hold what the workspace
 * was filled with (compared on bits); *buffer_index / *offset (either may be NULL): the first one -- the buffer of the layout it belongs to
 * and its offset from that buffer's end (>= 0), or from the first buffer's start (< 0: the guard in front of it); b2f_last_error names the
 * buffer.  0 without arena_guard, -1 on an error.                                                                                  */
B2F_API int b2f_arena_check(b2f_ctx *ctx, int *buffer_index, long long *offset);
/* b2f_guard_selftest: overwrites ONE guard word by a copy from the host, so that the checks can be seen to fire.  which = 0: offset +3
 * behind buffer 1 of the workspace's layout, 1: offset -2 in front of buffer 0 (both need arena_guard and a pass before; b2f_arena_check
 * then reports that word); 2 / 3: offset +2 behind / -1 in front of a guarded device buffer "selftest" as the b2f_op_* entries allocate
 * them -- the call then fails as such an entry fails, b2f_last_error naming the buffer, the side and the offset; 4 / 5: offset +2 behind
 * buffer "b" (1000 floats) / -1 in front of buffer "c" (7 bytes: 2 floats) of the staging scope those entries take their buffers from,
 * which holds "a" (10 floats), "b" and "c" and fails in the same words when it checks what it owns.                               */
B2F_API int b2f_guard_selftest(b2f_ctx *ctx, int which);
/* b2f_arena_plan: the workspace layout of a pass, computed on the host (no context, no device): the float offset of each of its 33 buffers
 * in the order img, tmp, cs[2..7], U[3..6], UB[3..6], cv, d[1..5], fs, bfs, logits, u2, flow_planar, ds[2..5] (0 for one the pass does
 * not have) and the total.  flags: 1 the full table, 2 a Soft model, 4 a sequence (B = T - 2), 8 a push of a stream, 16 with the past-flow
 * output.  Returns 33, or -1 with b2f_last_error set.                                                                              */
B2F_API int b2f_arena_plan(int arena_guard, int B, int H, int W, int flags, long long *offsets, int cap, long long *total);

#ifdef __cplusplus
}
#endif
#endif /* B2F_H */
