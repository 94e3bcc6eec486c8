// A stand-alone run of the host side of the fine-tuning objective of the Soft models (README.md:89-102; b2f::table_loss_ft_host of
// b2f_host.cpp, which runs b2f::table_loss_host of test.lua:266-297 first) for sanitizer builds: no GPU, no Python.  The stencil reaches
// one pixel to every side, so the first and last rows and columns are where it would read outside a plane: every tensor is allocated
// at its exact size.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/table_loss_ft_host_main.cpp -o tools/bin/table_loss_ft_host && tools/bin/table_loss_ft_host
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
    unsigned long long seed = 88172645463325252ull + (unsigned long long)(H * 131 + W * 7 + L + (past ? 1 : 0));
    auto fill = [&](size_t cnt, float lo, float hi) {
        own.emplace_back(new float[cnt]);   // exact size: ASan sees one element past the end
        float *p = own.back().get();
        for (size_t i = 0; i < cnt; ++i) {
            seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
            p[i] = lo + (hi - lo) * (float)(seed >> 40) / 16777216.0f;
        }
        return p;
    };
    for (int j = 0; j < L; ++j) {
        const size_t hw = (size_t)(H >> j) * (W >> j);
        for (int k = 0; k < per; ++k) {
            const bool img = k >= per - 2, occ = k == per - 3;
            float *p = fill((size_t)n * (img ? 3 : 2) * hw, occ ? 0.0f : -2.0f, occ ? 1.0f : 2.0f);
            if (!img && hw > 2) {   // non-finite values reach every branch
                p[1] = std::numeric_limits<float>::quiet_NaN();
                p[hw - 1] = occ ? 0.5f : std::numeric_limits<float>::infinity();
            }
            table.push_back(p);
        }
    }
    const float *ref = fill((size_t)n * 3 * H * W, -2.0f, 2.0f);
    std::vector<unsigned long long> loss((size_t)n * L * B2F_LOSS_FT_WORDS, 7ull), base((size_t)n * L * B2F_LOSS_WORDS, 7ull);
    int lv = 0;
    const char *why = b2f::table_loss_refusal(L * per, per, n, H, W, 20.0, &lv);
    if (why || lv != L) { fprintf(stderr, "refused: %s\n", why ? why : "level count"); return 1; }
    b2f::table_loss_ft_host(table.data(), L, past, n, H, W, ref, 20.0, loss.data());
    b2f::table_loss_host(table.data(), L, past, n, H, W, ref, 20.0, base.data());
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < L; ++j) {
            const unsigned long long *r = &loss[((size_t)b * L + j) * B2F_LOSS_FT_WORDS], *r0 = &base[((size_t)b * L + j) * B2F_LOSS_WORDS];
            const unsigned long long hw = (unsigned long long)(H >> j) * (W >> j);
            if (r[B2F_LOSS_PIXELS] != hw || r[15] != 0) { fprintf(stderr, "bad record\n"); return 1; }
            for (int d = 0; d < 2; ++d)
                if (r[B2F_LOSS_PHOTO_INSIDE + d] + r[B2F_LOSS_PHOTO_OUTSIDE + d] + r[B2F_LOSS_PHOTO_NONFINITE + d] != hw) { fprintf(stderr, "bad photo counts\n"); return 1; }
            for (int k = 0; k < B2F_LOSS_WORDS; ++k)
                if (r[k] != r0[k]) { fprintf(stderr, "word %d differs from the 16-word record\n", k); return 1; }
            if (r[B2F_LOSS_FT_SMOOTH2_FLOW_Q30] == 0 || (past != (r[B2F_LOSS_FT_SMOOTH2_PAST_Q30] != 0)) || r[B2F_LOSS_FT_SMOOTH2_NONFINITE] > hw ||
                r[B2F_LOSS_FT_GRAD_NONFINITE] > r[B2F_LOSS_PHOTO_INSIDE] + r[B2F_LOSS_PHOTO_INSIDE + 1]) { fprintf(stderr, "bad fine-tuning words\n"); return 1; }
        }
    printf("%d x %d, L = %d, %s, n = %d: smooth2_flow_q30[0][0] = %llu, ogx_q30[0][0][0] = %llu, smooth2_nonfinite[0][0] = %llu, grad_nonfinite[0][0] = %llu\n",
           H, W, L, past ? "soft" : "hard", n, loss[B2F_LOSS_FT_SMOOTH2_FLOW_Q30], loss[B2F_LOSS_FT_PHOTO_OGX_Q30], loss[B2F_LOSS_FT_SMOOTH2_NONFINITE],
           loss[B2F_LOSS_FT_GRAD_NONFINITE]);
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
    if (!rc) printf("table_loss_ft_host: ok\n");
    return rc;
}
