// Host check (no GPU): the item decode of conv3x3_wino6 divides by run-time values with the launcher's reciprocals -- (n * mul) >> sh with
// (mul, sh) = w6_div_magic(d), b2f_internal.h -- and that must equal n / d for every 0 <= n < 2^31.  Checks every n around the multiples of d
// that matter (the quotient steps at k d - 1 -> k d), the ends of the range and a pseudo-random sample, for every d up to 2^16, the powers of
// two and their neighbours, and random d up to 2^31 - 1.   hipcc --offload-arch=gfx950 -O2 -I back2future_amd/csrc tools/w6_div_check.hip && ./a.out
#include "b2f_internal.h"
#include <cstdio>
static unsigned long long bad = 0, done = 0;
static void check(int d)
{
    unsigned mul; int sh;
    b2f::w6_div_magic(d, &mul, &sh);
    auto one = [&](long long n) {
        if (n < 0 || n > 2147483647ll) return;
        const int q = (int)(((unsigned long long)(unsigned)n * mul) >> sh);
        ++done;
        if (q != (int)(n / d) && bad++ < 10) printf("n = %lld d = %d: %d, expected %lld\n", n, d, q, n / d);
    };
    const long long top = 2147483647ll, kmax = top / d;
    const long long ks[] = {0, 1, 2, 3, kmax / 3, kmax / 2, kmax - 1, kmax};
    for (long long k : ks)
        for (int e = -2; e <= 2; ++e) one(k * d + e);
    one(top); one(top - 1); one(top - d); one(top - d + 1);
    unsigned long long x = 88172645463325252ull + (unsigned)d;
    for (int i = 0; i < 64; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const long long n = (long long)(x & 0x7fffffffu);
        one(n); one(n - n % d); one(n - n % d - 1);
    }
}
int main()
{
    for (int d = 1; d <= 65536; ++d) check(d);
    for (int l = 1; l < 31; ++l)
        for (int e = -1; e <= 1; ++e) check((1 << l) + e);
    check(2147483647);
    unsigned long long x = 2463534242ull;
    for (int i = 0; i < 100000; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        check((int)(x % 2147483646ull) + 1);
    }
    printf("%llu quotients checked, %llu wrong\n", done, bad);
    return bad != 0;
}
