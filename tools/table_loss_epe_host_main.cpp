// A stand-alone run of the host side of the supervised objective (-optimize epe; train.lua:296-334 with criterions/L2Criterion.lua:27-71;
// b2f::table_loss_epe_host of b2f_host.cpp) for sanitizer builds: no GPU, no Python.  Level j reads the ground truth at (y << j, x << j):
// the last row and column of a level are where a wrong stride would read outside a plane, so every tensor is allocated at its exact size.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/table_loss_epe_host_main.cpp -o tools/bin/table_loss_epe_host && tools/bin/table_loss_epe_host
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
    std::vector<std::unique_ptr<unsigned char[]>> own8;
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
    auto bytes = [&](size_t cnt, unsigned mod) {
        own8.emplace_back(new unsigned char[cnt]);
        unsigned char *p = own8.back().get();
        for (size_t i = 0; i < cnt; ++i) p[i] = (unsigned char)((next() >> 33) % mod);
        return p;
    };
    for (int j = 0; j < L; ++j) {
        const size_t hw = (size_t)(H >> j) * (W >> j);
        for (int k = 0; k < per; ++k) {
            const bool img = k >= per - 2, occ = k == per - 3;
            const size_t cnt = (size_t)n * (img ? 3 : 2) * hw;
            float *p = fill(cnt, occ ? 0.0f : -2.0f, occ ? 1.0f : 2.0f);
            if (!img && hw > 2) {   // non-finite values reach every branch
                p[1] = std::numeric_limits<float>::quiet_NaN();
                p[hw - 1] = occ ? 0.5f : std::numeric_limits<float>::infinity();
            }
            table.push_back(p);
            grad.push_back(fill(cnt, 7.0f, 7.0f));
        }
    }
    const size_t HW = (size_t)H * W;
    float *gt = fill((size_t)n * 2 * HW, -40.0f, 40.0f);
    unsigned char *valid = bytes((size_t)n * HW, 3), *occ = bytes((size_t)n * HW, 5);
    for (size_t i = 0; i < (size_t)n * HW; ++i)
        if (!valid[i]) gt[(i / HW) * 2 * HW + i % HW] = (i & 1) ? 1e9f : std::numeric_limits<float>::quiet_NaN();
    int lv = 0;
    const char *why = b2f::table_loss_refusal(L * per, per, n, H, W, 20.0, &lv);
    if (why || lv != L) { fprintf(stderr, "refused: %s\n", why ? why : "level count"); return 1; }
    b2f_loss_epe_opts o;
    o.epe = 1.0; o.occ = 1.0; o.size_average = 0;
    const double lw[7] = {0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28};
    for (int j = 0; j < 7; ++j) o.level_weights[j] = lw[j];
    std::vector<double> given((size_t)L * 2, 3.0);
    std::vector<unsigned long long> first;
    for (int sa = 0; sa < 2; ++sa)
        for (int mode = 0; mode < 3; ++mode)
            for (int rescale = 0; rescale < 2; ++rescale)
                for (int with_valid = 0; with_valid < 2; ++with_valid) {
                    o.size_average = sa;
                    if ((why = b2f::loss_epe_refusal(o, gt, occ, mode, given.data(), L))) { fprintf(stderr, "refused: %s\n", why); return 1; }
                    std::vector<unsigned long long> loss((size_t)n * L * B2F_LOSS_EPE_WORDS, 7ull);
                    b2f::table_loss_epe_host(table.data(), L, past, n, H, W, gt, with_valid ? valid : nullptr, occ, 20.0, rescale != 0, o, mode,
                                             mode == B2F_EPE_COUNT_GIVEN ? given.data() : nullptr, loss.data(), grad.data());
                    for (int b = 0; b < n; ++b)
                        for (int j = 0; j < L; ++j) {
                            const unsigned long long *r = &loss[((size_t)b * L + j) * B2F_LOSS_EPE_WORDS];
                            const unsigned long long hw = (unsigned long long)(H >> j) * (W >> j);
                            if (r[B2F_LOSS_EPE_PIXELS] != hw || r[7] != 0 || r[B2F_LOSS_EPE_VALID] + r[B2F_LOSS_EPE_FLOW_NONFINITE] > hw ||
                                r[B2F_LOSS_EPE_LABELLED] + r[B2F_LOSS_EPE_OCC_NONFINITE] > hw ||
                                (!with_valid && r[B2F_LOSS_EPE_VALID] + r[B2F_LOSS_EPE_FLOW_NONFINITE] != hw)) { fprintf(stderr, "bad record\n"); return 1; }
                        }
                    for (size_t t = 0; t < grad.size(); ++t)   // the planes no term reaches are +0.0
                        if ((int)(t % per) != 0 && (int)(t % per) != per - 3 && grad[t][0] != 0.0f) { fprintf(stderr, "bad gradient plane\n"); return 1; }
                    if (first.empty()) first = loss;
                }
    // the records alone and the gradient alone
    std::vector<unsigned long long> loss((size_t)n * L * B2F_LOSS_EPE_WORDS, 7ull);
    o.size_average = 0;
    b2f::table_loss_epe_host(table.data(), L, past, n, H, W, gt, nullptr, occ, 20.0, false, o, 0, nullptr, loss.data(), nullptr);
    if (loss != first) { fprintf(stderr, "the records depend on the gradient\n"); return 1; }
    o.occ = 0.0;   // (occ > 0 without gt_occ is refused by the entry)
    b2f::table_loss_epe_host(table.data(), L, past, n, H, W, gt, valid, nullptr, 20.0, false, o, 0, nullptr, nullptr, grad.data());
    printf("%d x %d, L = %d, %s, n = %d: valid[0][0] = %llu, epe_q20[0][0] = %llu, flow_nonfinite[0][0] = %llu, labelled[0][0] = %llu, occ_q20[0][0] = %llu\n",
           H, W, L, past ? "soft" : "hard", n, first[B2F_LOSS_EPE_VALID], first[B2F_LOSS_EPE_Q20], first[B2F_LOSS_EPE_FLOW_NONFINITE],
           first[B2F_LOSS_EPE_LABELLED], first[B2F_LOSS_EPE_OCC_Q20]);
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
    if (!rc) printf("table_loss_epe_host: ok\n");
    return rc;
}
