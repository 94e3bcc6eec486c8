// A stand-alone run of the host side of the gradient table with the occlusion-aware SSIM + L1 photometric term
// (b2f::table_loss_grad_ssim_host of b2f_host.cpp: OSSIML1Criterion.lua:165-302) for sanitizer builds: no GPU, no Python.  The window
// reaches one pixel to every side, clamped to the plane, the second-order stencil two, so the first and last rows and columns are where
// it would read or write outside a plane: every tensor, input and output, is allocated at its exact size.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/table_loss_grad_ssim_host_main.cpp -o tools/bin/table_loss_grad_ssim_host && tools/bin/table_loss_grad_ssim_host
#include "b2f_host.h"
#include "../include/b2f.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

static b2f_loss_grad_ssim_opts defaults()
{
    // opts.lua:61-73, test.lua:29-31; first-order smoothness, OSSIML1
    b2f_loss_grad_ssim_opts o = {1.0, 1.0, 1.0, 0.1, 0.1, {0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28}, 0, 0, 0.85};
    return o;
}

// off: -1, or which of the five weights is 0; mode: B2F_SSIM_RANGE_*
static int run(int H, int W, int L, bool past, int n, bool size_average, bool second, double alpha, int mode, int off)
{
    const int per = past ? 5 : 4;
    std::vector<std::unique_ptr<float[]>> own;
    std::vector<const float *> table;
    std::vector<float *> grad;
    std::vector<size_t> count;
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
            const size_t cnt = (size_t)n * (img ? 3 : 2) * hw;
            float *p = fill(cnt, occ ? 0.0f : -2.0f, occ ? 1.0f : 2.0f);
            if (hw > 2) {   // non-finite values reach every branch: the flows, the occlusions and, through the range and the window, the images
                p[1] = std::numeric_limits<float>::quiet_NaN();
                p[hw - 1] = occ ? 0.5f : std::numeric_limits<float>::infinity();
            }
            table.push_back(p);
            own.emplace_back(new float[cnt]);
            grad.push_back(own.back().get());
            for (size_t i = 0; i < cnt; ++i) grad.back()[i] = 7.0f;
            count.push_back(cnt);
        }
    }
    const float *ref = fill((size_t)n * 3 * H * W, -2.0f, 2.0f);
    own.emplace_back(new float[(size_t)2 * L]);
    float *ranges = own.back().get();
    for (int j = 0; j < L; ++j) {
        ranges[2 * j] = -3.0f;
        ranges[2 * j + 1] = 3.0f;
    }
    int lv = 0;
    const char *why = b2f::table_loss_refusal(L * per, per, n, H, W, 20.0, &lv);
    if (why || lv != L) { fprintf(stderr, "refused: %s\n", why ? why : "level count"); return 1; }
    b2f_loss_grad_ssim_opts o = defaults();
    o.size_average = size_average ? 1 : 0;
    o.smooth_second_order = second ? 1 : 0;
    o.ssim_alpha = alpha;
    double *wt[5] = {&o.smooth_flow, &o.const_vel, &o.pme, &o.smooth_occ, &o.prior_occ};
    if (off >= 0) *wt[off] = 0.0;
    const float *given = mode == B2F_SSIM_RANGE_GIVEN ? ranges : nullptr;
    if (b2f::loss_grad_ssim_refusal(o) || b2f::ssim_range_refusal(mode, given)) { fprintf(stderr, "options refused\n"); return 1; }
    b2f::table_loss_grad_ssim_host(table.data(), L, past, n, H, W, ref, 20.0, b2f::loss_grad_ssim_base(o), o.ssim_alpha, mode, given, grad.data());
    size_t finite = 0, total = 0;
    double sum = 0.0;
    for (size_t t = 0; t < grad.size(); ++t)
        for (size_t i = 0; i < count[t]; ++i) {
            const float v = grad[t][i];
            ++total;
            if (std::isfinite(v)) { ++finite; sum += std::fabs((double)v); }
        }
    if (finite == 0 && H * W > 4) { fprintf(stderr, "no finite gradient element\n"); return 1; }
    if (off == 2) {   // without the photometric term the warped images' gradients are +0.0
        for (int j = 0; j < L; ++j)
            for (int k = per - 2; k < per; ++k)
                for (size_t i = 0; i < count[(size_t)j * per + k]; ++i)
                    if (grad[(size_t)j * per + k][i] != 0.0f || std::signbit(grad[(size_t)j * per + k][i])) { fprintf(stderr, "pme = 0 left a gradient\n"); return 1; }
    }
    printf("%d x %d, L = %d, %s, n = %d, size_average = %d, second order %d, alpha %g, range mode %d, weight %d off: %zu of %zu elements finite, sum |g| = %.9g\n",
           H, W, L, past ? "soft" : "hard", n, (int)size_average, (int)second, alpha, mode, off, finite, total, sum);
    return 0;
}

int main()
{
    int rc = 0;
    const double alphas[3] = {1.0, 0.85, 0.0};
    for (int past = 0; past < 2; ++past)
        for (int mode = B2F_SSIM_RANGE_BATCH; mode <= B2F_SSIM_RANGE_GIVEN; ++mode)
            for (int a = 0; a < 3; ++a) {
                const bool second = ((mode + a) & 1) != 0;
                rc |= run(1, 1, 1, past != 0, 2, false, second, alphas[a], mode, -1);
                rc |= run(3, 2, 1, past != 0, 2, true, second, alphas[a], mode, -1);
                rc |= run(48, 80, 5, past != 0, 2, a == 1, second, alphas[a], mode, -1);
            }
    for (int past = 0; past < 2; ++past)
        for (int off = 0; off < 5; ++off) rc |= run(48, 80, 5, past != 0, 2, false, off == 0, 0.85, B2F_SSIM_RANGE_GIVEN, off);
    b2f_loss_grad_ssim_opts bad = defaults();
    bad.ssim_alpha = 1.5;
    if (!b2f::loss_grad_ssim_refusal(bad)) { fprintf(stderr, "ssim_alpha = 1.5 was accepted\n"); rc = 1; }
    bad = defaults();
    bad.ssim_alpha = std::numeric_limits<double>::quiet_NaN();
    if (!b2f::loss_grad_ssim_refusal(bad)) { fprintf(stderr, "ssim_alpha = NaN was accepted\n"); rc = 1; }
    bad = defaults();
    bad.smooth_occ = -1.0;
    if (!b2f::loss_grad_ssim_refusal(bad)) { fprintf(stderr, "a negative weight was accepted\n"); rc = 1; }
    if (!rc) printf("table_loss_grad_ssim_host: ok\n");
    return rc;
}
