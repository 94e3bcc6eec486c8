// Host-only helpers shared by the C-ABI layer: canonical weight layout, deterministic
// init, the .t7 reader.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace b2f {

constexpr int kFeatH[8] = {0, 3, 16, 32, 64, 96, 128, 192};   // featMaps, pwc.lua:29,89
constexpr int kDecH[7] = {0, 128, 128, 96, 64, 32, 2};        // decoder(), pwc.lua:76-85
constexpr int kNDh = 162;

enum { KIND_FEAT = 0, KIND_OCC = 1, KIND_FLOW = 2, KIND_PAST = 3 };

struct ConvDesc {
    int kind;     // KIND_*
    int level;    // pyramid level (2..7 for features -- 1..7 with pwc_skip = 0 --, levels..l_st for decoders)
    int idx;      // conv index inside the unit (1..2 features, 1..6 decoders)
    int ci, co;   // Torch nInputPlane / nOutputPlane
    long long w_off, b_off;   // offsets into the flat canonical buffer
};

// The option table of createModelMulti (models/pwc.lua:88-121) that shapes the graph; frames = 3 is fixed.
// Defaults = the shipped models (opts.lua:83-98).
struct GraphOpts {
    int win = 9, levels = 7, skip = 2;
    int two_frame = 0, sum_cvs = 0, residual = 0, occ_input = 0, rescale_flow = 0;
    int siamese = 1;                                                               // pwc_siamese, pwc.lua:99,115
    bool past_flow = false;
    float flownet_factor = 20.f;
    int l_st() const { return skip + 1; }                                          // pwc.lua:136 (skip >= 0)
    // featMaps[l], pwc.lua:89,120-127: pwc_skip = 0 gives the level-1 unit featMaps[2] maps, pwc_siamese = 0 makes every level the image
    int feat(int l) const { return !siamese ? 3 : (l == 1 && skip == 0) ? kFeatH[2] : kFeatH[l]; }
    int feat_first() const { return skip == 0 ? 1 : 2; }                           // first level with a convUnit (pwc.lua:171-183)
    int nd() const { return win * win; }
    int nd_flow() const { return (two_frame || sum_cvs) ? nd() : 2 * nd(); }       // pwc.lua:254-285
    int nd_occ() const { return two_frame ? nd() : 2 * nd(); }
    int occ_in(int l) const                                                        // pwc.lua:288-305
    {
        int n = nd_occ() + feat(l) + (two_frame ? feat(l) : 0);
        if (l != levels) n += 2 + (occ_input ? 2 : 0);
        return n;
    }
    int flow_in(int l) const { return l == levels ? nd_flow() : nd_flow() + feat(l) + 2; }   // pwc.lua:325-337
    int n_outputs() const { return (levels - l_st() + 1) * (past_flow ? 5 : 4); }              // pwc.lua:459-489
    // the graph the fused fast path of b2f_api.hip is written for (any past_flow)
    bool shipped() const
    {
        return win == 9 && levels == 7 && skip == 2 && !two_frame && !sum_cvs && !residual && !occ_input && !rescale_flow &&
               siamese && flownet_factor == 20.f;
    }
    bool valid() const { return win >= 1 && (win & 1) && win <= 15 && levels >= 2 && levels <= 7 && skip >= 0 && skip + 1 <= levels; }
};
// "win=5,levels=4,skip=2,two_frame=0,sum_cvs=1,residual=1,occ_input=1,rescale_flow=1,flownet_factor=20" (any subset;
// also siamese=0|1 and the reference's option names pwc_ws, pwc_skip, pwc_sum_cvs, pwc_siamese).  past_flow is not set here (it comes with the weights).
bool parse_graph_opts(const char *text, GraphOpts &o, std::string &err);
std::string graph_opts_string(const GraphOpts &o);

std::vector<ConvDesc> weight_layout(const GraphOpts &o, long long *total);
long long param_count(const GraphOpts &o);
void random_weights(unsigned long long seed, const GraphOpts &o, float gain, float *out);
std::vector<ConvDesc> weight_layout(bool past_flow, long long *total);
long long param_count(bool past_flow);
void random_weights(unsigned long long seed, bool past_flow, float gain, float *out);

// xy2rgb of a planar n x 2 x H x W fp32 flow on the CPU (b2f_flowcolor.h per pixel; b2f_flow_rgb_host): rgb n x 3 x H x W bytes, or
// n x H x W x 3 with packed; max_norm > 0 = the maximum of every image, else each image's own; max_used: n doubles or nullptr
void flow_rgb_host(const float *flow, int n, int H, int W, double max_norm, bool packed, unsigned char *rgb, double *max_used);

// The scores of a planar n x 2 x H x W fp32 flow against ground truth on the CPU (b2f_flowscore.h per pixel; b2f_flow_score_host):
// scores n x B2F_SCORE_WORDS words; occ_prob, valid and gt_occ may be nullptr
void flow_score_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, const float *gt_flow,
                     const unsigned char *valid, const unsigned char *gt_occ, unsigned long long *scores);

// Motion compensation on the CPU (b2f_flowwarp.h per pixel; b2f_flow_warp_host): the two warped neighbours (n x 2 x 3 x H x W in the
// frames' element type, or nullptr) and the photometric records (n x B2F_PHOTO_WORDS words, or nullptr) of a planar n x 2 x H x W
// fp32 flow; im1 / im2 / im3: n x 3 x H x W each, bytes with bytes_in, floats otherwise; occ_prob may be nullptr.  past_flow (n x 2 x H x W
// or nullptr): the model's own past flow, which then places the past frame's samples instead of flow (b2f_flow_warp_past_host)
void flow_warp_host(const float *flow, const float *occ_prob, int n, int H, int W, double flow_scale, bool bytes_in, const void *im1,
                    const void *im2, const void *im3, void *warped, unsigned long long *photo, const float *past_flow = nullptr);

// The unsupervised validation loss of test.lua:266-297 on the CPU (b2f_tableloss.h per pixel; b2f_table_loss_host): table = L x (4 | 5)
// planar fp32 tensors in table order (per level f, [p,] o, iw1, iw3 at (H >> j) x (W >> j)), ref n x 3 x H x W, loss n x L x
// `words` words (B2F_LOSS_WORDS; a wider record keeps its further words zero)
void table_loss_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                     unsigned long long *loss, int words = 16);
// table_loss_host with records of B2F_LOSS_FT_WORDS words, and in words 16 .. 23 the fine-tuning terms of README.md:89-102
// (b2f_tableloss_ft.h per pixel; b2f_table_loss_ft_host)
void table_loss_ft_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                        unsigned long long *loss);
// table_loss_host with records of B2F_LOSS_SSIM_WORDS words, and in words 16 .. 25 the SSIM + L1 photometric sums and the ranges of
// criterions/OSSIML1Criterion.lua:47-163 (b2f_tableloss_ssim.h per pixel; b2f_table_loss_ssim_host); range_mode: B2F_SSIM_RANGE_*,
// ranges: L x 2 floats with B2F_SSIM_RANGE_GIVEN
void table_loss_ssim_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                          int range_mode, const float *ranges, unsigned long long *loss);
// what every *_ssim entry checks of its range (no HIP call): nullptr, or why not
const char *ssim_range_refusal(int range_mode, const float *ranges);
// the argument checks every table-loss entry shares (test.lua:266-297; no HIP call): nullptr and *L = n_outs / per, or why not
const char *table_loss_refusal(int n_outs, int per, int n, int H, int W, double flow_scale, int *L);
// what table_loss_refusal, and an entry that takes `per` from its context (b2f_ctx.h: level_size), says of a table of another size
constexpr char kTableSizeRefusal[] = "n_outs must be L x 4 (Hard) or L x 5 (Soft)";
// tensor t of a table of `per` tensors per level (f, [p,] o, iw1, iw3): its planes -- two for flows and occlusions, three for the warped
// images -- and its floats for n images of a table of H x W
inline int table_planes(int t, int per) { return t % per >= per - 2 ? 3 : 2; }
inline size_t table_floats(int t, int per, int n, int H, int W) { return (size_t)n * table_planes(t, per) * (H >> (t / per)) * (W >> (t / per)); }
// the level weights of opts.lua:61-73 (test.lua:29-31), the defaults of every objective's options
constexpr double kLossLevelWeights[7] = {0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28};
}  // namespace b2f
struct b2f_loss_grad_opts;
namespace b2f {
struct GradCoef;
// The gradient of the pme objective with respect to the output table on the CPU (train.lua:428-468; b2f_tableloss_grad.h per element;
// b2f_table_loss_grad_host): grad = the table's L x (4 | 5) tensors, every element written
void table_loss_grad_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                          const b2f_loss_grad_opts &opts, float *const *grad);
// nullptr, or why the options are refused (a negative or non-finite weight)
const char *loss_grad_refusal(const b2f_loss_grad_opts &o);
}  // namespace b2f
struct b2f_loss_grad_ft_opts;
namespace b2f {
struct GradFtCoef;
// The same with the fine-tuning criteria where the options' flags ask for them (b2f_tableloss_grad_ft.h per element;
// b2f_table_loss_grad_ft_host); with both flags 0 the bits of table_loss_grad_host, which calls it
void table_loss_grad_ft_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                             const b2f_loss_grad_ft_opts &opts, float *const *grad);
// nullptr, or why (as above, a pme_criterion outside {0, 1}, a negative or non-finite alpha, beta or gamma)
const char *loss_grad_ft_refusal(const b2f_loss_grad_ft_opts &o);
// the first-order options as fine-tuning options with both flags 0, and the first-order fields of fine-tuning options
b2f_loss_grad_ft_opts loss_grad_ft_from(const b2f_loss_grad_opts &o);
b2f_loss_grad_opts loss_grad_ft_base(const b2f_loss_grad_ft_opts &o);
void loss_grad_ft_coef(const b2f_loss_grad_ft_opts &o, int j, int h, int w, GradFtCoef *k);
}  // namespace b2f
struct b2f_loss_grad_ssim_opts;
namespace b2f {
struct GradSsimCoef;
// The same with the SSIM + L1 photometric term of criterions/OSSIML1Criterion.lua:165-302 (b2f_tableloss_grad_ssim.h per element;
// b2f_table_loss_grad_ssim_host): opts' first-order fields and smooth_second_order (pme_criterion is not read), alpha and the range
void table_loss_grad_ssim_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                               const b2f_loss_grad_ft_opts &opts, double ssim_alpha, int range_mode, const float *ranges, float *const *grad);
// nullptr, or why (as loss_grad_refusal, an ssim_alpha outside [0, 1] or NaN)
const char *loss_grad_ssim_refusal(const b2f_loss_grad_ssim_opts &o);
// the fields the SSIM + L1 options share with the fine-tuning options (pme_criterion 0, alpha = beta = gamma = 1)
b2f_loss_grad_ft_opts loss_grad_ssim_base(const b2f_loss_grad_ssim_opts &o);
void loss_grad_ssim_coef(const b2f_loss_grad_ft_opts &o, double ssim_alpha, int j, int h, int w, GradSsimCoef *k);
// words RANGE_OWN and RANGE_USED of records of B2F_LOSS_SSIM_WORDS words (OSSIML1Criterion.lua:62-67), every other word left alone
void ssim_ranges_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, int range_mode, const float *ranges,
                      unsigned long long *loss);
// the coefficients of level j of h x w (include/b2f.h: k_s .. k_pr) and which terms are evaluated
void loss_grad_coef(const b2f_loss_grad_opts &o, int j, int h, int w, GradCoef *k);
}  // namespace b2f
struct b2f_loss_grad_plain_opts;
namespace b2f {
struct GradPlainCoef;
// table_loss_host with records of B2F_LOSS_PLAIN_WORDS words, and in words 16 .. 29 the photometric sums without occlusion masking of
// criterions/MBCCriterion.lua:35-102 and MSSIML1Criterion.lua:45-153 and the ranges of the latter's lines 63-68 (b2f_tableloss_plain.h
// per pixel; b2f_table_loss_plain_host)
void table_loss_plain_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                           int range_mode, const float *ranges, unsigned long long *loss);
// words RANGE_OWN and RANGE_USED of records of B2F_LOSS_PLAIN_WORDS words: the range over R_j, the warped images, the occlusions and, on
// Soft tables, the past flow (MSSIML1Criterion.lua:63-68); every other word left alone
void plain_ranges_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, int range_mode, const float *ranges,
                       unsigned long long *loss);
// The gradient table with those photometric terms (MBCCriterion.lua:104-186, MSSIML1Criterion.lua:155-261; b2f_tableloss_plain.h per
// element; b2f_table_loss_grad_plain_host): opts as for table_loss_grad_ssim_host, criterion B2F_PLAIN_*, penalty B2F_PLAIN_*
void table_loss_grad_plain_host(const float *const *table, int L, bool past, int n, int H, int W, const float *ref, double flow_scale,
                                const b2f_loss_grad_ft_opts &opts, int criterion, int penalty, double ssim_alpha, int range_mode, const float *ranges,
                                float *const *grad);
// nullptr, or why (as loss_grad_ssim_refusal, a criterion or penalty that is none of B2F_PLAIN_*, the quadratic penalty without BCC)
const char *loss_grad_plain_refusal(const b2f_loss_grad_plain_opts &o);
b2f_loss_grad_ft_opts loss_grad_plain_base(const b2f_loss_grad_plain_opts &o);
void loss_grad_plain_coef(const b2f_loss_grad_ft_opts &o, int criterion, int penalty, double ssim_alpha, int j, int h, int w, GradPlainCoef *k);
}  // namespace b2f
struct b2f_loss_epe_opts;
namespace b2f {
// The supervised objective on the CPU (train.lua:296-334, criterions/L2Criterion.lua:27-71; b2f_tableloss_epe.h per pixel;
// b2f_table_loss_epe_host): gt_flow n x 2 x H x W, valid / gt_occ n x H x W bytes or nullptr, read at (y << j, x << j); loss n x L x
// B2F_LOSS_EPE_WORDS words and grad the table's L x (4 | 5) tensors, each or nullptr; counts: L x 2 doubles with B2F_EPE_COUNT_GIVEN
void table_loss_epe_host(const float *const *table, int L, bool past, int n, int H, int W, const float *gt_flow, const unsigned char *valid,
                         const unsigned char *gt_occ, double flow_scale, bool rescale, const b2f_loss_epe_opts &opts, int count_mode,
                         const double *counts, unsigned long long *loss, float *const *grad);
// nullptr, or why the *_epe entries refuse their options, ground truth or counts (no HIP call)
const char *loss_epe_refusal(const b2f_loss_epe_opts &o, const void *gt_flow, const void *gt_occ, int count_mode, const double *counts, int L);
// epe * lw_j and occ * lw_j of level j (train.lua:313-314,328-331; lw_j = 1 with size_average, train.lua:60-64)
void loss_epe_base(const b2f_loss_epe_opts &o, int j, double *kf, double *ko);
// the valid and the labelled source pixels of every image and level: cnt n x L x 2
void epe_counts_host(const unsigned char *valid, const unsigned char *gt_occ, int L, int n, int H, int W, unsigned long long *cnt);

// .t7 reader (b2f_t7.cpp): returns false and fills err on failure.
bool load_t7(const std::string &path, std::vector<float> &flat, bool &past_flow, std::string &err);
// any graph shape: infer = true takes win / levels / skip from the file, false checks the file against g (see b2f_t7.cpp)
bool load_t7_ex(const std::string &path, GraphOpts &g, bool infer, std::vector<float> &flat, std::string &err);

}  // namespace b2f
