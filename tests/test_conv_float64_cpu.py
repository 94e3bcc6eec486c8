"""CPU: tests/conv_float64.py against itself, before any kernel is held to it.

The float64 Winograd of every algorithm reproduces conv64 (the matrices are right); the float32 emulation of every algorithm stays inside
bound() on every family and every shape the GPU file runs (the reference alone meets the bar) and its worst err / (u S_direct) per algorithm
and family is the recorded table the GPU file reads; three mutations of the emulation -- U rounded to bf16, one tap dropped, two input
channels of a chunk swapped -- turn the check red; S = 0 gives exactly 0 and an all-zero image exactly the bias."""
import numpy as np
import pytest

from tests import conv_float64 as F

WINO = ("F2", "F4", "F6", "1D")
TEETH_SHAPE = {"direct": (40, 12, 17, 33), "direct-b": (40, 12, 17, 33), "F2": (72, 68, 17, 33), "F4": (72, 68, 17, 33), "F6": (72, 68, 17, 33), "1D": (72, 68, 17, 33)}


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("alg", WINO)
def test_float64_winograd_is_the_convolution(alg, leaky):
    for shape in [(3, 2, 12, 12), (9, 5, 1, 1), (8, 4, 13, 49), (5, 3, 17, 7)]:
        for family in ("gauss", "sparse"):
            x, w, b = F.make_case(family, 7, 2, *shape)
            ref = F.conv64(x, w, b, 1, leaky)
            got = F.winograd(x, w, b, alg, "64", leaky)
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (alg, shape, family)


def test_yardsticks_dominate_the_result():
    """|conv64| <= S_direct <= S_wino (|G| |g| |G^T| etc. only add), and the medians of S_wino / S_direct: ~7, ~60, ~225"""
    x, w, b = F.make_case("gauss", 3, 2, 64, 32, 24, 24)
    Sd = F.S_direct(x, w, b)
    assert (np.abs(F.conv64(x, w, b)) <= Sd * (1 + 1e-12)).all()
    for alg, lo, hi in (("F2", 4, 12), ("F4", 30, 120), ("F6", 100, 450), ("1D", 4, 30)):
        Sw = F.S_wino(x, w, b, alg)
        assert (Sw >= Sd * (1 - 1e-12)).all(), alg
        assert lo < np.median(Sw / Sd) < hi, (alg, float(np.median(Sw / Sd)))


@pytest.mark.parametrize("alg", F.ALGS)
def test_emulation_meets_the_bound_and_is_the_recorded_table(alg):
    """every family at every shape of EMULATED: err <= n u S of the algorithm; the worst err / (u S_direct) per family is what
    tests/golden/conv_float64_ratios.json records (python -m tests.conv_float64 rewrites it)"""
    failures = []
    for family in F.FAMILIES:
        worst, worst_own = 0.0, 0.0
        for s in F.EMULATED[alg]:
            r_direct, r_alg, n = F.emulation_case(alg, family, s[:4], s[4])
            worst, worst_own = max(worst, r_direct), max(worst_own, r_alg)
            if not r_alg <= n:
                failures.append("%s %s %s: err = %.2f u S, bound n = %d" % (alg, family, s, r_alg, n))
        print("%-8s %-8s worst err / (u S_direct) = %10.2f, err / (u S) = %8.3f" % (alg, family, worst, worst_own))
        for got, own in ((worst, False), (worst_own, True)):
            rec = F.recorded(alg, family, own)
            if not abs(got - rec) <= 1e-3 * rec + 1e-6:
                failures.append("%s %s: worst ratio %.6g, recorded %.6g" % (alg, family, got, rec))
    assert not failures, "\n".join(failures)


def test_head_emulation_meets_its_bound_and_is_the_recorded_table():
    """two chained float32 convolutions against head64: inside the carried bound on every family and map, the worst err / (u S2) recorded"""
    failures = []
    for family in F.FAMILIES:
        cases = [F.head_emulation_case(family, H, W) for H, W in F.HEAD]
        worst, rec = max(c[0] for c in cases), F.recorded("head", family)
        print("head     %-8s worst err / (u S2) = %8.3f, worst err / bound = %.4f" % (family, worst, max(c[1] for c in cases)))
        if not max(c[1] for c in cases) <= 1.0:
            failures.append("head %s: the emulation is at %.3f of the bound" % (family, max(c[1] for c in cases)))
        if not abs(worst - rec) <= 1e-3 * rec + 1e-6:
            failures.append("head %s: worst ratio %.6g, recorded %.6g" % (family, worst, rec))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mutate", ["bf16", "tap", "swap"])
@pytest.mark.parametrize("alg", F.ALGS)
def test_mutations_turn_the_check_red(alg, mutate):
    """the GPU file's check -- the rigorous bound, and err / (u S_direct) and err / (u S of the algorithm) within 2 x the recorded ratios -- must fail a subtly wrong kernel"""
    shape = TEETH_SHAPE[alg]
    for family in ("gauss", "outlier"):
        good_direct, good_alg, n = F.emulation_case(alg, family, shape, 1)
        bar, bar_own = 2.0 * F.recorded(alg, family), 2.0 * F.recorded(alg, family, True)
        assert good_alg <= min(n, bar_own) and good_direct <= bar, (alg, family, "the unmutated emulation fails")
        r_direct, r_alg, n = F.emulation_case(alg, family, shape, 1, mutate)
        print("%-6s %-5s %-8s err / (u S_direct) = %.3g (bar %.3g), err / (u S) = %.3g (bar %.3g, bound %d)" % (alg, mutate, family, r_direct, bar, r_alg, bar_own, n))
        assert r_alg > n or r_direct > bar or r_alg > bar_own, (alg, mutate, family, r_direct, bar)


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("alg", F.ALGS)
def test_zero_products_give_exact_results(alg, leaky):
    """sparse: the last image is all zero and every other bias is zero.  Where every product is zero the result is exactly the bias
    (through the kernels' LeakyReLU), exactly 0 where the bias is zero too."""
    shape = (40, 36, 8, 16)
    x, w, b = F.make_case("sparse", 11, 2, *shape)
    got = F.emulate(alg, x, w, b, 1, leaky)
    S0 = F.yardstick(alg, x, w, np.zeros_like(b))
    quiet = S0 == 0
    assert quiet[-1].all() and (b[0::2] == 0).all()
    exp = np.broadcast_to(F.round32_leaky(b, leaky)[None, :, None, None], got.shape)
    np.testing.assert_array_equal(got[quiet], exp[quiet])
    assert (got[-1, 0::2] == 0).all()


def test_integers_are_exact_on_the_dyadic_paths():
    """integers: the direct and F(2x2) emulations give conv64 bit for bit (through round32_leaky); F(4x4), F(6x6) and the 1-D form have thirds in G"""
    for alg, shape, stride in (("direct", (40, 12, 17, 33), 1), ("direct-b", (40, 36, 9, 33), 2), ("F2", (200, 96, 13, 49), 1)):
        x, w, b = F.make_case("integers", F.SEED, 2, *shape)
        exact = F.conv64(x, w, b, stride, False)
        assert (exact.astype(np.float32).astype(np.float64) == exact).all()
        for leaky in (False, True):
            np.testing.assert_array_equal(F.emulate(alg, x, w, b, stride, leaky), F.round32_leaky(exact, leaky), err_msg=alg)


def test_normalised_first_layer_emulation_meets_its_bound_and_is_the_recorded_table():
    failures = []
    for family in F.FAMILIES:
        cases = [F.first_norm_emulation_case(family, sh) for sh in F.FIRST]
        worst, n, rec = max(c[0] for c in cases), cases[0][1], F.recorded("first-norm", family)
        print("first-norm %-8s worst err / (u S_direct) = %8.3f (n = %d)" % (family, worst, n))
        if not worst <= n:
            failures.append("first-norm %s: err = %.2f u S, bound n = %d" % (family, worst, n))
        if not abs(worst - rec) <= 1e-3 * rec + 1e-6:
            failures.append("first-norm %s: worst ratio %.6g, recorded %.6g" % (family, worst, rec))
    assert not failures, "\n".join(failures)
