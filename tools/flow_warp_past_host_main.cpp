// A stand-alone run of the host side of motion compensation with the model's own past flow (pwc.lua:425-432, OBCCriterion.lua:80-81;
// b2f::flow_warp_host of b2f_host.cpp with past_flow) for sanitizer builds: no GPU, no Python.  The taps right of and below the last
// column and row are where the warp would read past a plane, so every tensor is allocated at its exact size, and the past flow carries
// targets far outside the image, NaN and +-Inf of its own.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I back2future_amd/csrc back2future_amd/csrc/b2f_host.cpp tools/flow_warp_past_host_main.cpp -o tools/bin/flow_warp_past_host && tools/bin/flow_warp_past_host
#include "b2f_host.h"
#include "../include/b2f.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

template <typename T>
static int run(int H, int W, int n, bool with_prob)
{
    const size_t hw = (size_t)H * W;
    unsigned long long seed = 88172645463325252ull + (unsigned long long)(H * 131 + W * 7 + n + sizeof(T));
    auto next = [&]() {
        seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
        return (float)(seed >> 40) / 16777216.0f;
    };
    auto floats = [&](size_t cnt, float lo, float hi) {
        std::unique_ptr<float[]> p(new float[cnt]);   // exact size: ASan sees one element past the end
        for (size_t i = 0; i < cnt; ++i) p[i] = lo + (hi - lo) * next();
        return p;
    };
    auto flow = floats((size_t)n * 2 * hw, -0.6f, 0.6f), past = floats((size_t)n * 2 * hw, -0.6f, 0.6f), prob = floats((size_t)n * 2 * hw, 0.0f, 1.0f);
    const float far = (float)(H + W + 5) / 20.0f, specials[5] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                                                                   -std::numeric_limits<float>::infinity(), far, -far};
    for (size_t i = 0; i < (size_t)n * 2 * hw; i += 7) past[i] = specials[(i / 7) % 5];
    for (size_t i = 3; i < (size_t)n * 2 * hw; i += 11) flow[i] = specials[(i / 11) % 5];
    // whole-pixel targets on the last column and row for k = -20
    for (int x = 0; x < W && H > 3; ++x) {
        past[(size_t)3 * W + x] = -(float)(W - 1 - x) / 20.0f;
        past[hw + (size_t)3 * W + x] = -(float)(H - 1 - 3) / 20.0f;
    }
    std::unique_ptr<T[]> im[3];
    for (auto &p : im) {
        p.reset(new T[(size_t)n * 3 * hw]);
        for (size_t i = 0; i < (size_t)n * 3 * hw; ++i) p[i] = sizeof(T) == 1 ? (T)(next() * 255.0f) : (T)next();
    }
    std::unique_ptr<T[]> warped(new T[(size_t)n * 6 * hw]), plain(new T[(size_t)n * 6 * hw]);
    std::vector<unsigned long long> photo((size_t)n * B2F_PHOTO_WORDS, 7ull), photo_plain((size_t)n * B2F_PHOTO_WORDS, 7ull);
    const float *pp = with_prob ? prob.get() : nullptr;
    b2f::flow_warp_host(flow.get(), pp, n, H, W, 20.0, sizeof(T) == 1, im[0].get(), im[1].get(), im[2].get(), warped.get(), photo.data(), past.get());
    b2f::flow_warp_host(flow.get(), pp, n, H, W, 20.0, sizeof(T) == 1, im[0].get(), im[1].get(), im[2].get(), plain.get(), photo_plain.data());
    for (int b = 0; b < n; ++b) {
        const unsigned long long *r = &photo[(size_t)b * B2F_PHOTO_WORDS], *q = &photo_plain[(size_t)b * B2F_PHOTO_WORDS];
        for (int d = 0; d < 2; ++d)
            if (r[B2F_PHOTO_INSIDE + d] + r[B2F_PHOTO_OUTSIDE + d] + r[B2F_PHOTO_NONFINITE + d] != hw) { fprintf(stderr, "bad counts\n"); return 1; }
        for (int k = 1; k < B2F_PHOTO_WORDS; k += 2)   // the future direction does not see the past flow
            if (r[k] != q[k]) { fprintf(stderr, "the future half differs\n"); return 1; }
        if (memcmp(warped.get() + ((size_t)b * 2 + 1) * 3 * hw, plain.get() + ((size_t)b * 2 + 1) * 3 * hw, 3 * hw * sizeof(T))) { fprintf(stderr, "the future planes differ\n"); return 1; }
    }
    // the flow as its own past flow: the plain call's bytes and words; the outputs alone
    b2f::flow_warp_host(flow.get(), pp, n, H, W, 20.0, sizeof(T) == 1, im[0].get(), im[1].get(), im[2].get(), warped.get(), photo.data(), flow.get());
    if (memcmp(warped.get(), plain.get(), (size_t)n * 6 * hw * sizeof(T)) || photo != photo_plain) { fprintf(stderr, "past_flow == flow differs from the plain call\n"); return 1; }
    b2f::flow_warp_host(flow.get(), pp, n, H, W, 20.0, sizeof(T) == 1, im[0].get(), im[1].get(), im[2].get(), nullptr, photo.data(), past.get());
    b2f::flow_warp_host(flow.get(), pp, n, H, W, 20.0, sizeof(T) == 1, im[0].get(), im[1].get(), im[2].get(), warped.get(), nullptr, past.get());
    printf("%d x %d, n = %d, %s frames, occ_prob %d: inside %llu / %llu, outside %llu / %llu, nonfinite %llu / %llu\n", H, W, n,
           sizeof(T) == 1 ? "byte" : "float", (int)with_prob, photo[B2F_PHOTO_INSIDE], photo[B2F_PHOTO_INSIDE + 1], photo[B2F_PHOTO_OUTSIDE],
           photo[B2F_PHOTO_OUTSIDE + 1], photo[B2F_PHOTO_NONFINITE], photo[B2F_PHOTO_NONFINITE + 1]);
    return 0;
}

int main()
{
    int rc = 0;
    for (int with_prob = 0; with_prob < 2; ++with_prob) {
        const int sizes[4][2] = {{1, 1}, {5, 7}, {33, 61}, {64, 64}};
        for (const auto &s : sizes) {
            rc |= run<float>(s[0], s[1], 2, with_prob != 0);
            rc |= run<unsigned char>(s[0], s[1], 2, with_prob != 0);
        }
    }
    if (!rc) printf("flow_warp_past_host: ok\n");
    return rc;
}
