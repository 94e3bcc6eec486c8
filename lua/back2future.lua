----------------------------------------------------------------------------
-- back2future.lua -- drop-in replacement of the reference's inference module
-- (/root/reference/back2future.lua) on top of libb2f.so (MI355X / gfx950).
--
--   back2future = require('back2future')
--   computeFlow = back2future.init('Ours-Soft-ft-KITTI')
--   flow, fwd_occ, bwd_occ = computeFlow(im1, im2, im3)
--
-- local computeFlow, computeFlowSequence = back2future.init(opt): the second closure takes a whole video; the third and
-- fourth (computeFlowBatchF32, computeFlowSequenceF32) return float flows and, on request, the occlusion probabilities.
-- Same module table (init, normalize), same argument and return order and types
-- as back2future.lua:45-130: im* are 3xHxW torch tensors in [0,1] (image.load),
-- flow is a 2xHxW torch.DoubleTensor, the masks are 1xHxW torch.ByteTensor.
-- Needs LuaJIT (ffi) and torch7's CPU tensors only: no cutorch / cunn / cudnn /
-- nngraph / stn / spy.  The model directory convention ('models/RoamingImages_*.t7'
-- relative to the current directory, back2future.lua:100-110) is implemented inside
-- b2f_init.
--
-- NOTE: this build image has no LuaJIT / Torch7, so this file is shipped UNTESTED;
-- back2future_amd/back2future.py is the tested mirror of the same calls
-- (INTEGRATION.md).
----------------------------------------------------------------------------
local ffi = require 'ffi'
require 'torch'

ffi.cdef[[
typedef struct b2f_ctx b2f_ctx;
const char *b2f_last_error(void);
int  b2f_init(const char *name_or_path, int device, b2f_ctx **out);
void b2f_destroy(b2f_ctx *ctx);
int  b2f_info(const b2f_ctx *ctx, int *levels, int *win, int *past_flow, int *n_outputs, long long *n_params);
int  b2f_compute_flow(b2f_ctx *ctx, const float *im1, const float *im2, const float *im3,
                      int H0, int W0, double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_compute_flow_sequence(b2f_ctx *ctx, int T, const float *frames, int H0, int W0,
                               double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_compute_flow_sequence_u8(b2f_ctx *ctx, int T, const unsigned char *frames, int H0, int W0,
                                  double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_compute_flow_batch_f32(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                int H0, int W0, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_compute_flow_sequence_f32(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                   float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_compute_flow_device(b2f_ctx *ctx, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                             int H0, int W0, float *dev_flow, float *dev_occ_prob,
                             unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
int  b2f_compute_flow_sequence_device(b2f_ctx *ctx, int T, int in_kind, const void *dev_frames, int H0, int W0,
                                      float *dev_flow, float *dev_occ_prob,
                                      unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
enum { B2F_RGB_PLANAR = 0, B2F_RGB_PACKED = 1 };
int b2f_flow_rgb_host(const float *flow, int n, int H, int W, double max_norm, int layout,
                      unsigned char *rgb, double *max_used);
int b2f_flow_rgb_device(b2f_ctx *ctx, const float *dev_flow, int n, int H, int W, double max_norm, int layout,
                        unsigned char *dev_rgb, double *dev_max_used, void *stream);
int b2f_op_flow_rgb(b2f_ctx *ctx, const float *flow, int n, int H, int W, double max_norm, int layout,
                    unsigned char *rgb, double *max_used);
int b2f_compute_flow_batch_rgb(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                               int H0, int W0, double max_norm, int layout, unsigned char *rgb, double *max_used,
                               float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_compute_flow_sequence_rgb(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                  double max_norm, int layout, unsigned char *rgb, double *max_used,
                                  float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
typedef struct b2f_stream b2f_stream;
int  b2f_stream_open(b2f_ctx *ctx, int cams, int in_kind, int H0, int W0, b2f_stream **out);
void b2f_stream_close(b2f_stream *st);
int  b2f_stream_reset(b2f_stream *st);
int  b2f_stream_info(const b2f_stream *st, int *cams, int *H0, int *W0, int *in_kind, long long *pushed);
int  b2f_stream_push(b2f_stream *st, const void *frames, float *flow, float *occ_prob,
                     unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready);
int  b2f_stream_push_rgb(b2f_stream *st, const void *frames, double max_norm, int layout, unsigned char *rgb,
                         double *max_used, float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ, int *ready);
int  b2f_stream_push_device(b2f_stream *st, const void *dev_frames, float *dev_flow, float *dev_occ_prob,
                            unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream, int *ready);
enum {
    B2F_SCORE_PIXELS = 0,
    B2F_SCORE_EPE_Q20 = 4,
    B2F_SCORE_OUTLIERS = 8,
    B2F_SCORE_OCC = 12,
    B2F_SCORE_NONFINITE = 21,
    B2F_SCORE_WORDS = 22
};
int b2f_flow_score_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                        const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                        unsigned long long *scores);
int b2f_flow_score_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W,
                          double flow_scale, const float *dev_gt_flow, const unsigned char *dev_valid,
                          const unsigned char *dev_gt_occ, unsigned long long *dev_scores, void *stream);
int b2f_op_flow_score(b2f_ctx *ctx, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                      const float *gt_flow, const unsigned char *valid, const unsigned char *gt_occ,
                      unsigned long long *scores);
int b2f_compute_flow_batch_score(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                 int H0, int W0, double flow_scale, const float *gt_flow, const unsigned char *valid,
                                 const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                 unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_compute_flow_sequence_score(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                    double flow_scale, const float *gt_flow, const unsigned char *valid,
                                    const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                    unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_flow_warp_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, int in_kind,
                       const void *im1, const void *im2, const void *im3, void *warped, unsigned long long *photo);
int b2f_flow_warp_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_occ_prob, int n, int H, int W,
                         double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                         void *dev_warped, unsigned long long *dev_photo, void *stream);
int b2f_op_flow_warp(b2f_ctx *ctx, const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale,
                     int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                     unsigned long long *photo);
int b2f_compute_flow_batch_warp(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                int H0, int W0, double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_compute_flow_sequence_warp(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                   double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                   float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* the past flow of a Soft model (skip_ubfs[3]) and motion compensation with it (include/b2f.h) */
int b2f_forward_device_past(b2f_ctx *ctx, const void *dev_in, int in_kind, int B, int H, int W, float *dev_flow,
                            float *dev_past_flow, float *dev_occ, float *dev_est3, void *stream);
int b2f_forward_sequence_device_past(b2f_ctx *ctx, const void *dev_frames, int in_kind, int T, int H, int W, float *dev_flow,
                                     float *dev_past_flow, float *dev_occ, float *dev_est3, void *stream);
int b2f_compute_flow_batch_past(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                int H0, int W0, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                unsigned char *bwd_occ);
int b2f_compute_flow_sequence_past(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0, float *flow,
                                   float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_compute_flow_device_past(b2f_ctx *ctx, int n, int in_kind, const void *dev_im1, const void *dev_im2, const void *dev_im3,
                                 int H0, int W0, float *dev_flow, float *dev_past_flow, float *dev_occ_prob,
                                 unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
int b2f_compute_flow_sequence_device_past(b2f_ctx *ctx, int T, int in_kind, const void *dev_frames, int H0, int W0,
                                          float *dev_flow, float *dev_past_flow, float *dev_occ_prob,
                                          unsigned char *dev_fwd_occ, unsigned char *dev_bwd_occ, void *stream);
int b2f_flow_warp_past_host(const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W,
                            double flow_scale, int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                            unsigned long long *photo);
int b2f_flow_warp_past_device(b2f_ctx *ctx, const float *dev_flow, const float *dev_past_flow, const float *dev_occ_prob, int n,
                              int H, int W, double flow_scale, int in_kind, const void *dev_im1, const void *dev_im2,
                              const void *dev_im3, void *dev_warped, unsigned long long *dev_photo, void *stream);
int b2f_op_flow_warp_past(b2f_ctx *ctx, const float *flow, const float *past_flow, const float *occ_prob, int n, int H, int W,
                          double flow_scale, int in_kind, const void *im1, const void *im2, const void *im3, void *warped,
                          unsigned long long *photo);
int b2f_compute_flow_batch_warp_past(b2f_ctx *ctx, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                     int H0, int W0, double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                     float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_compute_flow_sequence_warp_past(b2f_ctx *ctx, int T, int in_kind, const void *frames, int H0, int W0,
                                        double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                        float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
/* the unsupervised validation loss of test.lua:266-297 on the output table (include/b2f.h, B2F_LOSS_*) */
int b2f_table_loss_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                        double flow_scale, unsigned long long *loss);
int b2f_table_loss_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                          double flow_scale, unsigned long long *dev_loss, void *stream);
int b2f_op_table_loss(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                      double flow_scale, unsigned long long *loss);
int b2f_forward_loss(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                     float **outs, int n_outs);
int b2f_forward_loss_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                            unsigned long long *dev_loss, void *stream);
/* ... with the fine-tuning terms of README.md:89-102 in words 16 .. 23 of records of 24 words (include/b2f.h, B2F_LOSS_FT_*) */
int b2f_table_loss_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                           double flow_scale, unsigned long long *loss);
int b2f_table_loss_ft_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                             double flow_scale, unsigned long long *dev_loss, void *stream);
int b2f_op_table_loss_ft(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                         double flow_scale, unsigned long long *loss);
int b2f_forward_loss_ft(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                        float **outs, int n_outs);
int b2f_forward_loss_ft_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                               unsigned long long *dev_loss, void *stream);
/* ... with the SSIM + L1 sums of criterions/OSSIML1Criterion.lua in words 16 .. 25 of records of 32 words (include/b2f.h, B2F_LOSS_SSIM_*);
   range_mode: 0 the batch's range, 1 each image's own, 2 `ranges` (L x 2 floats) */
int b2f_table_loss_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                             double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
int b2f_table_loss_ssim_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                               double flow_scale, unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
int b2f_op_table_loss_ssim(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                           double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
int b2f_forward_loss_ssim(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                          float **outs, int n_outs, int range_mode, const float *ranges);
int b2f_forward_loss_ssim_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                 unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
int b2f_loss_ssim_weights(double out[2]);
/* the gradient of the pme objective with respect to the output table: gradOutputs of train.lua:279-472 (include/b2f.h) */
typedef struct b2f_loss_grad_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;
    double level_weights[7];
    int size_average;
} b2f_loss_grad_opts;
int b2f_loss_grad_defaults(b2f_loss_grad_opts *opts);
int b2f_table_loss_grad_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                             double flow_scale, const b2f_loss_grad_opts *opts, float *const *grad);
int b2f_table_loss_grad_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                               const float *dev_ref, double flow_scale, const b2f_loss_grad_opts *opts, float *const *dev_grad,
                               void *stream);
int b2f_op_table_loss_grad(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                           double flow_scale, const b2f_loss_grad_opts *opts, float *const *grad);
int b2f_forward_loss_grad(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, const b2f_loss_grad_opts *opts,
                          unsigned long long *loss, float *const *grad, int n_outs, float *const *outs);
int b2f_forward_loss_grad_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                 const b2f_loss_grad_opts *opts, unsigned long long *dev_loss, float *const *dev_grad, int n_outs,
                                 void *stream);
/* the same for the Soft models' fine-tuning objective: -smooth_second_order, -pme_criterion OBGCC (include/b2f.h) */
typedef struct b2f_loss_grad_ft_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;
    double level_weights[7];
    int size_average;
    int smooth_second_order;
    int pme_criterion;
    double pme_alpha, pme_beta, pme_gamma;
} b2f_loss_grad_ft_opts;
int b2f_loss_grad_ft_defaults(b2f_loss_grad_ft_opts *opts);
int b2f_table_loss_grad_ft_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                double flow_scale, const b2f_loss_grad_ft_opts *opts, float *const *grad);
int b2f_table_loss_grad_ft_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                  const float *dev_ref, double flow_scale, const b2f_loss_grad_ft_opts *opts,
                                  float *const *dev_grad, void *stream);
int b2f_op_table_loss_grad_ft(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                              double flow_scale, const b2f_loss_grad_ft_opts *opts, float *const *grad);
int b2f_forward_loss_grad_ft(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                             const b2f_loss_grad_ft_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                             float *const *outs);
int b2f_forward_loss_grad_ft_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                    const b2f_loss_grad_ft_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                    int n_outs, void *stream);
typedef struct b2f_loss_grad_ssim_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;
    double level_weights[7];
    int size_average;
    int smooth_second_order;
    double ssim_alpha;
} b2f_loss_grad_ssim_opts;
int b2f_loss_grad_ssim_defaults(b2f_loss_grad_ssim_opts *opts);
int b2f_table_loss_grad_ssim_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                  double flow_scale, const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode,
                                  const float *ranges);
int b2f_table_loss_grad_ssim_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                    const float *dev_ref, double flow_scale, const b2f_loss_grad_ssim_opts *opts,
                                    float *const *dev_grad, void *stream, int range_mode, const float *ranges);
int b2f_op_table_loss_grad_ssim(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                                double flow_scale, const b2f_loss_grad_ssim_opts *opts, float *const *grad, int range_mode,
                                const float *ranges);
int b2f_forward_loss_grad_ssim(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                               const b2f_loss_grad_ssim_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                               float *const *outs, int range_mode, const float *ranges);
int b2f_forward_loss_grad_ssim_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                      const b2f_loss_grad_ssim_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                      int n_outs, void *stream, int range_mode, const float *ranges);
int b2f_table_loss_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                              double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
int b2f_table_loss_plain_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W, const float *dev_ref,
                                double flow_scale, unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
int b2f_op_table_loss_plain(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                            double flow_scale, unsigned long long *loss, int range_mode, const float *ranges);
int b2f_forward_loss_plain(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                           float **outs, int n_outs, int range_mode, const float *ranges);
int b2f_forward_loss_plain_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                  unsigned long long *dev_loss, void *stream, int range_mode, const float *ranges);
typedef struct b2f_loss_grad_plain_opts {
    double smooth_flow, const_vel, pme, smooth_occ, prior_occ;
    double level_weights[7];
    int size_average;
    int smooth_second_order;
    int criterion;
    int penalty;
    double ssim_alpha;
} b2f_loss_grad_plain_opts;
int b2f_loss_grad_plain_defaults(b2f_loss_grad_plain_opts *opts);
int b2f_table_loss_grad_plain_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *ref,
                                   double flow_scale, const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode,
                                   const float *ranges);
int b2f_table_loss_grad_plain_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                                     const float *dev_ref, double flow_scale, const b2f_loss_grad_plain_opts *opts,
                                     float *const *dev_grad, void *stream, int range_mode, const float *ranges);
int b2f_op_table_loss_grad_plain(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *ref,
                                 double flow_scale, const b2f_loss_grad_plain_opts *opts, float *const *grad, int range_mode,
                                 const float *ranges);
int b2f_forward_loss_grad_plain(b2f_ctx *ctx, const float *x, int n, int H, int W, double flow_scale,
                                const b2f_loss_grad_plain_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                float *const *outs, int range_mode, const float *ranges);
int b2f_forward_loss_grad_plain_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, double flow_scale,
                                       const b2f_loss_grad_plain_opts *opts, unsigned long long *dev_loss, float *const *dev_grad,
                                       int n_outs, void *stream, int range_mode, const float *ranges);
typedef struct b2f_loss_epe_opts {
    double epe;
    double occ;
    int size_average;
    double level_weights[7];
} b2f_loss_epe_opts;
int b2f_loss_epe_defaults(b2f_loss_epe_opts *opts);
int b2f_table_loss_epe_host(const float *const *table, int n_outs, int n, int H, int W, int past_flow, const float *gt_flow,
                            const unsigned char *valid, const unsigned char *gt_occ, double flow_scale, int rescale,
                            const b2f_loss_epe_opts *opts, int count_mode, const double *counts, unsigned long long *loss,
                            float *const *grad);
int b2f_table_loss_epe_device(b2f_ctx *ctx, const float *const *dev_table, int n_outs, int n, int H, int W,
                              const float *dev_gt_flow, const unsigned char *dev_valid, const unsigned char *dev_gt_occ,
                              double flow_scale, const b2f_loss_epe_opts *opts, int count_mode, const double *counts,
                              unsigned long long *dev_loss, float *const *dev_grad, void *stream);
int b2f_op_table_loss_epe(b2f_ctx *ctx, const float *const *table, int n_outs, int n, int H, int W, const float *gt_flow,
                          const unsigned char *valid, const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts,
                          int count_mode, const double *counts, unsigned long long *loss, float *const *grad);
int b2f_forward_loss_epe(b2f_ctx *ctx, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                         const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode,
                         const double *counts, unsigned long long *loss, float *const *grad, int n_outs, float *const *outs);
int b2f_forward_loss_epe_device(b2f_ctx *ctx, const void *dev_in, int in_kind, int n, int H, int W, const float *dev_gt_flow,
                                const unsigned char *dev_valid, const unsigned char *dev_gt_occ, double flow_scale,
                                const b2f_loss_epe_opts *opts, int count_mode, const double *counts, unsigned long long *dev_loss,
                                float *const *dev_grad, int n_outs, void *stream);
typedef struct b2f_multi b2f_multi;
int  b2f_init_multi(const char *name_or_path, int n_gpus, const int *devices, b2f_multi **out);
void b2f_destroy_multi(b2f_multi *m);
int  b2f_multi_compute_flow_batch(b2f_multi *m, int n, const float *im1, const float *im2, const float *im3,
                                  int H0, int W0, double *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_multi_compute_flow_batch_f32(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                      int H0, int W0, float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int  b2f_multi_compute_flow_sequence_f32(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                         float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_batch_rgb(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                     int H0, int W0, double max_norm, int layout, unsigned char *rgb, double *max_used,
                                     float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_sequence_rgb(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                        double max_norm, int layout, unsigned char *rgb, double *max_used,
                                        float *flow, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_batch_score(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                       int H0, int W0, double flow_scale, const float *gt_flow, const unsigned char *valid,
                                       const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                       unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_sequence_score(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                          double flow_scale, const float *gt_flow, const unsigned char *valid,
                                          const unsigned char *gt_occ, unsigned long long *scores, float *flow,
                                          unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_batch_warp(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                      int H0, int W0, double flow_scale, void *warped, unsigned long long *photo,
                                      float *flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_sequence_warp(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                         double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                         float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_batch_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                      int H0, int W0, float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                      unsigned char *bwd_occ);
int b2f_multi_compute_flow_sequence_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0, float *flow,
                                         float *past_flow, float *occ_prob, unsigned char *fwd_occ, unsigned char *bwd_occ);
int b2f_multi_compute_flow_batch_warp_past(b2f_multi *m, int n, int in_kind, const void *im1, const void *im2, const void *im3,
                                           int H0, int W0, double flow_scale, void *warped, unsigned long long *photo,
                                           float *flow, float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                           unsigned char *bwd_occ);
int b2f_multi_compute_flow_sequence_warp_past(b2f_multi *m, int T, int in_kind, const void *frames, int H0, int W0,
                                              double flow_scale, void *warped, unsigned long long *photo, float *flow,
                                              float *past_flow, float *occ_prob, unsigned char *fwd_occ,
                                              unsigned char *bwd_occ);
int b2f_multi_forward_loss(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss);
int b2f_multi_forward_loss_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss);
int b2f_multi_forward_loss_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                                int range_mode, const float *ranges);
int b2f_multi_forward_loss_grad(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                const b2f_loss_grad_opts *opts, unsigned long long *loss, float *const *grad, int n_outs);
int b2f_multi_forward_loss_grad_ft(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                   const b2f_loss_grad_ft_opts *opts, unsigned long long *loss, float *const *grad, int n_outs);
int b2f_multi_forward_loss_grad_ssim(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                     const b2f_loss_grad_ssim_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                     int range_mode, const float *ranges);
int b2f_multi_forward_loss_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale, unsigned long long *loss,
                                 int range_mode, const float *ranges);
int b2f_multi_forward_loss_grad_plain(b2f_multi *m, const float *x, int n, int H, int W, double flow_scale,
                                      const b2f_loss_grad_plain_opts *opts, unsigned long long *loss, float *const *grad, int n_outs,
                                      int range_mode, const float *ranges);
int b2f_multi_forward_loss_epe(b2f_multi *m, const float *x, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                               const unsigned char *gt_occ, double flow_scale, const b2f_loss_epe_opts *opts, int count_mode,
                               const double *counts, unsigned long long *loss, float *const *grad, int n_outs);
]]

local lib = ffi.load(os.getenv('B2F_LIB') or 'libb2f.so')

local M = {}

local meanstd = {
   mean = { 0.485, 0.456, 0.406 },
   std = { 0.229, 0.224, 0.225 },
}

local function check(rc)
   if rc ~= 0 then error(ffi.string(lib.b2f_last_error())) end   -- THError -> Lua error, as in the reference
end

-- M.normalize = TF.ColorNormalize(meanstd)  (back2future.lua:42-45, transforms.lua:33-45)
local function normalize(imgs)
   local img = imgs:clone()
   local chs = (img:size(1) / 3) - 1
   for c = 0, chs do
      for i = 1, 3 do
         img[3 * c + i]:add(-meanstd.mean[i])
         img[3 * c + i]:div(meanstd.std[i])
      end
   end
   return img
end
M.normalize = normalize

local function init(opt)
   opt = opt or 'Ours-Soft-ft-KITTI'
   local pctx = ffi.new('b2f_ctx*[1]')
   check(lib.b2f_init(opt, tonumber(os.getenv('B2F_DEVICE') or 0), pctx))
   local ctx = ffi.gc(pctx[0], lib.b2f_destroy)

   -- `channels` is a global in the reference (back2future.lua:120-126); kept for scripts that read it
   channels = 9

   local computeFlow = function(im1, im2, im3)
      local a, b, c = im1:float():contiguous(), im2:float():contiguous(), im3:float():contiguous()
      assert(a:dim() == 3 and a:size(1) == 3, 'expected 3 x H x W images')
      assert(a:isSameSizeAs(b) and a:isSameSizeAs(c), 'the three frames must have the same size')
      local height, width = a:size(2), a:size(3)
      print(width - math.fmod(width, 64), height - math.fmod(height, 64))   -- back2future.lua:69
      local flow_est = torch.DoubleTensor(2, height, width)
      local fwd_occ_est = torch.ByteTensor(1, height, width)
      local bwd_occ_est = torch.ByteTensor(1, height, width)
      check(lib.b2f_compute_flow(ctx, a:data(), b:data(), c:data(), height, width,
                                 flow_est:data(), fwd_occ_est:data(), bwd_occ_est:data()))
      return flow_est, fwd_occ_est, bwd_occ_est
   end

   -- a video: frames is a T x 3 x H x W tensor (FloatTensor in [0,1], or ByteTensor: value = byte / 255); returns the
   -- (T-2) x 2 x H x W flow and (T-2) x 1 x H x W masks, entry i = computeFlow(frames[i], frames[i+1], frames[i+2])
   local computeFlowSequence = function(frames)
      assert(frames:dim() == 4 and frames:size(2) == 3, 'expected T x 3 x H x W frames')
      local T, height, width = frames:size(1), frames:size(3), frames:size(4)
      assert(T >= 3, 'a sequence needs T >= 3 frames')
      local flow_est = torch.DoubleTensor(T - 2, 2, height, width)
      local fwd_occ_est = torch.ByteTensor(T - 2, 1, height, width)
      local bwd_occ_est = torch.ByteTensor(T - 2, 1, height, width)
      if torch.type(frames) == 'torch.ByteTensor' then
         local f = frames:contiguous()
         check(lib.b2f_compute_flow_sequence_u8(ctx, T, f:data(), height, width,
                                                flow_est:data(), fwd_occ_est:data(), bwd_occ_est:data()))
      else
         local f = frames:float():contiguous()
         check(lib.b2f_compute_flow_sequence(ctx, T, f:data(), height, width,
                                             flow_est:data(), fwd_occ_est:data(), bwd_occ_est:data()))
      end
      return flow_est, fwd_occ_est, bwd_occ_est
   end

   -- float outputs (b2f_compute_flow_batch_f32 / _sequence_f32): the flow is a FloatTensor, computeFlow's DoubleTensor
   -- rounded to float, never widened; with want_occ_prob a 4th result holds the n x 2 x H x W occlusion probabilities.
   -- Frames: FloatTensors in [0,1] or, all of them, ByteTensors (value = byte / 255).
   local function frames_of(...)
      local ts, bytes = {...}, true
      for _, t in ipairs(ts) do bytes = bytes and torch.type(t) == 'torch.ByteTensor' end
      for i, t in ipairs(ts) do ts[i] = bytes and t:contiguous() or t:float():contiguous() end
      return ts, bytes and 2 or 1   -- B2F_IN_U8 / B2F_IN_UNIT
   end
   local function f32_outputs(n, height, width, want_occ_prob)
      return torch.FloatTensor(n, 2, height, width), torch.ByteTensor(n, 1, height, width),
             torch.ByteTensor(n, 1, height, width), want_occ_prob and torch.FloatTensor(n, 2, height, width) or nil
   end
   local computeFlowBatchF32 = function(im1, im2, im3, want_occ_prob)
      local ts, kind = frames_of(im1, im2, im3)
      local a, b, c = ts[1], ts[2], ts[3]
      assert(a:dim() == 4 and a:size(2) == 3, 'expected n x 3 x H x W batches')
      assert(a:isSameSizeAs(b) and a:isSameSizeAs(c), 'the three frame batches must have the same size')
      local n, height, width = a:size(1), a:size(3), a:size(4)
      local flow_est, fwd_occ_est, bwd_occ_est, occ_prob = f32_outputs(n, height, width, want_occ_prob)
      check(lib.b2f_compute_flow_batch_f32(ctx, n, kind, a:data(), b:data(), c:data(), height, width, flow_est:data(),
                                           occ_prob and occ_prob:data() or nil, fwd_occ_est:data(), bwd_occ_est:data()))
      return flow_est, fwd_occ_est, bwd_occ_est, occ_prob
   end
   local computeFlowSequenceF32 = function(frames, want_occ_prob)
      local ts, kind = frames_of(frames)
      local f = ts[1]
      assert(f:dim() == 4 and f:size(2) == 3, 'expected T x 3 x H x W frames')
      local T, height, width = f:size(1), f:size(3), f:size(4)
      assert(T >= 3, 'a sequence needs T >= 3 frames')
      local flow_est, fwd_occ_est, bwd_occ_est, occ_prob = f32_outputs(T - 2, height, width, want_occ_prob)
      check(lib.b2f_compute_flow_sequence_f32(ctx, T, kind, f:data(), height, width, flow_est:data(),
                                              occ_prob and occ_prob:data() or nil, fwd_occ_est:data(), bwd_occ_est:data()))
      return flow_est, fwd_occ_est, bwd_occ_est, occ_prob
   end
   -- frames that arrive one at a time (a camera, a decoder): openStream(height, width[, cams[, bytes]]) returns a table with
   -- push(frames[, want_occ_prob]) -> nil for the first two pushes, then flow, fwd_occ, bwd_occ[, occ_prob] of the triplet
   -- (k-2, k-1, k) with a leading cams axis (FloatTensor flow, as computeFlowBatchF32), reset() and close().  frames:
   -- cams x 3 x H x W (3 x H x W with one camera), FloatTensor in [0,1] or, with bytes = true, ByteTensor.
   local openStream = function(height, width, cams, bytes)
      cams = cams or 1
      local pst = ffi.new('b2f_stream*[1]')
      check(lib.b2f_stream_open(ctx, cams, bytes and 2 or 1, height, width, pst))
      -- the finalizer captures ctx: the context cannot be collected (and b2f_destroy cannot close the stream under it) before the
      -- stream's own finalizer has run
      local st = ffi.gc(pst[0], function(p) lib.b2f_stream_close(p); ctx = nil end)
      local S = {}
      function S.push(frames, want_occ_prob)
         assert((torch.type(frames) == 'torch.ByteTensor') == (bytes and true or false),
                bytes and 'this stream takes ByteTensor frames' or 'this stream takes float frames in [0,1], not a ByteTensor')
         local f = bytes and frames:contiguous() or frames:float():contiguous()
         assert(f:nElement() == cams * 3 * height * width, 'expected cams x 3 x H x W frames')
         local flow_est, fwd_occ_est, bwd_occ_est, occ_prob = f32_outputs(cams, height, width, want_occ_prob)
         local ready = ffi.new('int[1]')
         check(lib.b2f_stream_push(st, f:data(), flow_est:data(), occ_prob and occ_prob:data() or nil, fwd_occ_est:data(),
                                   bwd_occ_est:data(), ready))
         if ready[0] == 0 then return nil end
         return flow_est, fwd_occ_est, bwd_occ_est, occ_prob
      end
      function S.reset() check(lib.b2f_stream_reset(st)) end
      function S.framesPushed()
         local n = ffi.new('long long[1]')
         check(lib.b2f_stream_info(st, nil, nil, nil, nil, n))
         return tonumber(n[0])
      end
      function S.close()
         if st then lib.b2f_stream_close(ffi.gc(st, nil)); st = nil end
      end
      return S
   end
   return computeFlow, computeFlowSequence, computeFlowBatchF32, computeFlowSequenceF32, openStream
end
M.init = init

-- Several GPUs of one node (replaces nn.DataParallelTable, util.lua:27-48): initMulti(opt, nGPU) returns
-- computeFlowBatch(im1, im2, im3) on n x 3 x H x W tensors; the n triplets are split over the GPUs by the
-- library, the weights are broadcast to every GPU once (RCCL).  nGPU = 0: all visible GPUs.
local function initMulti(opt, nGPU)
   opt = opt or 'Ours-Soft-ft-KITTI'
   local pm = ffi.new('b2f_multi*[1]')
   check(lib.b2f_init_multi(opt, nGPU or 0, nil, pm))
   local m = ffi.gc(pm[0], lib.b2f_destroy_multi)
   return function(im1, im2, im3)
      local a, b, c = im1:float():contiguous(), im2:float():contiguous(), im3:float():contiguous()
      assert(a:dim() == 4 and a:size(2) == 3, 'expected n x 3 x H x W batches')
      assert(a:isSameSizeAs(b) and a:isSameSizeAs(c), 'the three frame batches must have the same size')
      local n, height, width = a:size(1), a:size(3), a:size(4)
      local flow_est = torch.DoubleTensor(n, 2, height, width)
      local fwd_occ_est = torch.ByteTensor(n, 1, height, width)
      local bwd_occ_est = torch.ByteTensor(n, 1, height, width)
      check(lib.b2f_multi_compute_flow_batch(m, n, a:data(), b:data(), c:data(), height, width,
                                             flow_est:data(), fwd_occ_est:data(), bwd_occ_est:data()))
      return flow_est, fwd_occ_est, bwd_occ_est
   end
end
M.initMulti = initMulti

return M
