// A stand-alone run of the host side of the photometric terms without occlusion masking (criterions/MBCCriterion.lua:35-186,
// criterions/MSSIML1Criterion.lua:45-261; b2f::table_loss_plain_host and b2f::table_loss_grad_plain_host of b2f_host.cpp) for sanitizer
// builds: no GPU, no Python.  The 3 x 3 window with replication and the five-point cross are where a wrong clamp would read outside a
// plane, and the range pass reads two further tensors, so every tensor is allocated at its exact size.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/table_loss_plain_host_main.cpp -o tools/bin/table_loss_plain_host && tools/bin/table_loss_plain_host
#include "b2f_host.h"
#include "../include/b2f.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

static int run(int H, int W, int L, bool past, int n)
{
    const int per = past ? 5 : 4;
    std::vector<std::unique_ptr<float[]>> own;
    std::vector<const float *> table;
    std::vector<float *> grad;
    unsigned long long seed = 88172645463325252ull + (unsigned long long)(H * 131 + W * 7 + L + (past ? 1 : 0));
    auto next = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    auto fill = [&](size_t cnt, float lo, float hi) {
        own.emplace_back(new float[cnt]);   // exact size: ASan sees one element past the end
        float *p = own.back().get();
        for (size_t i = 0; i < cnt; ++i) p[i] = lo + (hi - lo) * (float)(next() >> 40) / 16777216.0f;
        return p;
    };
    for (int j = 0; j < L; ++j) {
        const size_t hw = (size_t)(H >> j) * (W >> j);
        for (int k = 0; k < per; ++k) {
            const bool img = k >= per - 2, occ = k == per - 3;
            const size_t cnt = (size_t)n * (img ? 3 : 2) * hw;
            float *p = fill(cnt, occ ? 0.0f : img ? -2.0f : -0.2f, occ ? 1.0f : img ? 2.0f : 0.2f);
            if (hw > 2) {   // non-finite values reach every branch: NaN and Inf in the flows, the occlusions and the images of image 0
                p[1] = std::numeric_limits<float>::quiet_NaN();
                p[hw - 1] = occ ? 0.5f : std::numeric_limits<float>::infinity();
            }
            table.push_back(p);
            grad.push_back(fill(cnt, 7.0f, 7.0f));
        }
    }
    float *ref = fill((size_t)n * 3 * H * W, -2.0f, 2.0f);
    if ((size_t)H * W > 2) ref[(size_t)H * W + 1] = std::numeric_limits<float>::quiet_NaN();
    int lv = 0;
    const char *why = b2f::table_loss_refusal(L * per, per, n, H, W, 20.0, &lv);
    if (why || lv != L) { fprintf(stderr, "refused: %s\n", why ? why : "level count"); return 1; }
    std::vector<float> given((size_t)L * 2);
    for (int j = 0; j < L; ++j) { given[2 * j] = -3.0f; given[2 * j + 1] = 3.0f; }
    std::vector<unsigned long long> base((size_t)n * L * B2F_LOSS_WORDS, 7ull), first;
    b2f::table_loss_host(table.data(), L, past, n, H, W, ref, 20.0, base.data());
    for (int mode = 0; mode < 3; ++mode) {
        const float *ranges = mode == B2F_SSIM_RANGE_GIVEN ? given.data() : nullptr;
        if ((why = b2f::ssim_range_refusal(mode, ranges))) { fprintf(stderr, "refused: %s\n", why); return 1; }
        std::vector<unsigned long long> loss((size_t)n * L * B2F_LOSS_PLAIN_WORDS, 7ull);
        b2f::table_loss_plain_host(table.data(), L, past, n, H, W, ref, 20.0, mode, ranges, loss.data());
        for (int b = 0; b < n; ++b)
            for (int j = 0; j < L; ++j) {
                const unsigned long long *r = &loss[((size_t)b * L + j) * B2F_LOSS_PLAIN_WORDS], *r16 = &base[((size_t)b * L + j) * B2F_LOSS_WORDS];
                for (int k = 0; k < B2F_LOSS_WORDS; ++k)
                    if (r[k] != r16[k]) { fprintf(stderr, "word %d differs from b2f_table_loss_host's\n", k); return 1; }
                for (int k = 30; k < B2F_LOSS_PLAIN_WORDS; ++k)
                    if (r[k]) { fprintf(stderr, "reserved word %d is not 0\n", k); return 1; }
                for (int d = 0; d < 2; ++d)
                    if (r[B2F_LOSS_PLAIN_SSIM_NONFINITE + d] > r[B2F_LOSS_PHOTO_INSIDE + d]) { fprintf(stderr, "bad record\n"); return 1; }
            }
        if (first.empty()) first = loss;
        for (int crit = 0; crit < 2; ++crit)
            for (int pen = 0; pen < (crit == B2F_PLAIN_BCC ? 2 : 1); ++pen)
                for (int no_occ = 0; no_occ < 2; ++no_occ)
                    for (int second = 0; second < 2; ++second) {
                        b2f_loss_grad_plain_opts o;
                        o.smooth_flow = 1.0; o.const_vel = 1.0; o.pme = 1.0; o.smooth_occ = no_occ ? 0.0 : 0.1; o.prior_occ = no_occ ? 0.0 : 0.1;
                        const double lw[7] = {0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28};
                        for (int j = 0; j < 7; ++j) o.level_weights[j] = lw[j];
                        o.size_average = second; o.smooth_second_order = second; o.criterion = crit; o.penalty = pen; o.ssim_alpha = second ? 1.0 : 0.85;
                        if ((why = b2f::loss_grad_plain_refusal(o))) { fprintf(stderr, "refused: %s\n", why); return 1; }
                        b2f::table_loss_grad_plain_host(table.data(), L, past, n, H, W, ref, 20.0, b2f::loss_grad_plain_base(o), o.criterion, o.penalty,
                                                        o.ssim_alpha, mode, ranges, grad.data());
                        for (size_t t = 0; t < grad.size(); ++t)   // -no_occ: the occlusion planes are +0.0
                            if (no_occ && (int)(t % per) == per - 3 && (grad[t][0] != 0.0f || std::signbit(grad[t][0]))) { fprintf(stderr, "bad occlusion plane\n"); return 1; }
                    }
    }
    printf("%d x %d, L = %d, %s, n = %d: l1[0][0] = %llu, sq[0][0] = %llu, ssim[0][0] = %llu, l1n[0][0] = %llu, nonfinite[0][0] = %llu\n", H, W, L,
           past ? "soft" : "hard", n, first[B2F_LOSS_PLAIN_L1_Q30], first[B2F_LOSS_PLAIN_SQ_Q30], first[B2F_LOSS_PLAIN_SSIM_Q30],
           first[B2F_LOSS_PLAIN_L1N_Q30], first[B2F_LOSS_PLAIN_SSIM_NONFINITE]);
    return 0;
}

int main()
{
    int rc = 0;
    for (int past = 0; past < 2; ++past) {
        rc |= run(1, 1, 1, past != 0, 2);
        rc |= run(3, 2, 1, past != 0, 2);
        rc |= run(48, 80, 5, past != 0, 2);
    }
    if (!rc) printf("table_loss_plain_host: ok\n");
    return rc;
}
