// A stand-alone run of the host side of the occlusion-aware SSIM + L1 photometric term (criterions/OSSIML1Criterion.lua:47-163;
// b2f::table_loss_ssim_host of b2f_host.cpp, which runs b2f::table_loss_host of test.lua:266-297 first) for sanitizer builds: no GPU, no
// Python.  The window reaches one pixel to every side with its indices clamped to the plane, so the first and last rows and columns
// are where it would read outside: every tensor is allocated at its exact size.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/table_loss_ssim_host_main.cpp -o tools/bin/table_loss_ssim_host && tools/bin/table_loss_ssim_host
#include "b2f_host.h"
#include "../include/b2f.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

static float as_float(unsigned long long w)
{
    const unsigned u = (unsigned)w;
    float v;
    std::memcpy(&v, &u, sizeof v);
    return v;
}

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
            // flows of a tenth of a pixel at scale 20: most targets stay inside
            float *p = fill((size_t)n * (img ? 3 : 2) * hw, occ ? 0.0f : img ? -2.0f : -0.005f, occ ? 1.0f : img ? 2.0f : 0.005f);
            if (hw > 2) {   // non-finite values reach every branch: a NaN in a window, an infinity in the range of image 0
                p[1] = std::numeric_limits<float>::quiet_NaN();
                if (!occ && j == L - 1) p[hw - 1] = std::numeric_limits<float>::infinity();
            }
            table.push_back(p);
        }
    }
    const float *ref = fill((size_t)n * 3 * H * W, -2.0f, 2.0f);
    int lv = 0;
    const char *why = b2f::table_loss_refusal(L * per, per, n, H, W, 20.0, &lv);
    if (why || lv != L) { fprintf(stderr, "refused: %s\n", why ? why : "level count"); return 1; }
    std::vector<unsigned long long> base((size_t)n * L * B2F_LOSS_WORDS, 7ull);
    b2f::table_loss_host(table.data(), L, past, n, H, W, ref, 20.0, base.data());
    std::vector<float> given((size_t)L * 2);
    for (int j = 0; j < L; ++j) { given[2 * j] = -2.5f; given[2 * j + 1] = 2.5f; }
    unsigned long long any_sum = 0, any_nonf = 0;
    for (int mode = B2F_SSIM_RANGE_BATCH; mode <= B2F_SSIM_RANGE_GIVEN; ++mode) {
        if (b2f::ssim_range_refusal(mode, mode == B2F_SSIM_RANGE_GIVEN ? given.data() : nullptr)) { fprintf(stderr, "range refused\n"); return 1; }
        std::vector<unsigned long long> loss((size_t)n * L * B2F_LOSS_SSIM_WORDS, 7ull);
        b2f::table_loss_ssim_host(table.data(), L, past, n, H, W, ref, 20.0, mode, mode == B2F_SSIM_RANGE_GIVEN ? given.data() : nullptr, loss.data());
        for (int b = 0; b < n; ++b)
            for (int j = 0; j < L; ++j) {
                const unsigned long long *r = &loss[((size_t)b * L + j) * B2F_LOSS_SSIM_WORDS], *r0 = &base[((size_t)b * L + j) * B2F_LOSS_WORDS];
                for (int k = 0; k < B2F_LOSS_WORDS; ++k)
                    if (r[k] != r0[k]) { fprintf(stderr, "word %d differs from the 16-word record\n", k); return 1; }
                for (int k = 26; k < B2F_LOSS_SSIM_WORDS; ++k)
                    if (r[k]) { fprintf(stderr, "reserved word %d is not 0\n", k); return 1; }
                for (int d = 0; d < 2; ++d) {
                    if (r[B2F_LOSS_SSIM_NONFINITE + d] > r[B2F_LOSS_PHOTO_INSIDE + d]) { fprintf(stderr, "more non-finite than inside\n"); return 1; }
                    if (r[B2F_LOSS_SSIM_Q30 + d] > 16ull * r[B2F_LOSS_PHOTO_INSIDE + d] << 30) { fprintf(stderr, "sum beyond saturation\n"); return 1; }
                    any_sum += r[B2F_LOSS_SSIM_Q30 + d] + r[B2F_LOSS_SSIM_L1N_Q30 + d];
                    any_nonf += r[B2F_LOSS_SSIM_NONFINITE + d];
                }
                const float mn = as_float(r[B2F_LOSS_SSIM_RANGE_OWN]), mx = as_float(r[B2F_LOSS_SSIM_RANGE_OWN + 1]);
                if (!(mn <= mx) || (r[B2F_LOSS_SSIM_RANGE_OWN] >> 32) || (r[B2F_LOSS_SSIM_RANGE_USED] >> 32)) { fprintf(stderr, "bad range words\n"); return 1; }
                if (mode == B2F_SSIM_RANGE_IMAGE && (r[22] != r[24] || r[23] != r[25])) { fprintf(stderr, "image mode does not use the own range\n"); return 1; }
                if (mode == B2F_SSIM_RANGE_GIVEN && (as_float(r[22]) != -2.5f || as_float(r[23]) != 2.5f)) { fprintf(stderr, "given range not used\n"); return 1; }
            }
        printf("%d x %d, L = %d, %s, n = %d, mode %d: ssim_q30[0][0] = %llu %llu, l1n_q30[0][0] = %llu %llu, nonfinite[0][0] = %llu %llu, used %g .. %g\n", H, W, L,
               past ? "soft" : "hard", n, mode, loss[16], loss[17], loss[18], loss[19], loss[20], loss[21], (double)as_float(loss[22]), (double)as_float(loss[23]));
    }
    if (H * W > 6 && (!any_sum || !any_nonf)) { fprintf(stderr, "the sums or the non-finite count were never reached\n"); return 1; }
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
    if (!rc) printf("table_loss_ssim_host: ok\n");
    return rc;
}
