"""CPU: tests/conv_float64.py against itself, before any kernel is held to it.

The float64 Winograd of every algorithm reproduces conv64 (the matrices are right); the float32 emulation of every algorithm stays inside
bound() on every family and every shape the GPU file runs (the reference alone meets the bar) and its worst err / (u S_direct) per algorithm
and family is the recorded table the GPU file reads; three mutations of the emulation -- U rounded to bf16, one tap dropped, two input
channels of a chunk swapped -- turn the check red; S = 0 gives exactly 0 and an all-zero image exactly the bias.  The tile-geometry sweep
of tests/test_gpu_conv_edges.py: the shapes generated from conv_float64.GEOMETRY hold every residue and block edge, the emulations meet
the bound on them, and two mutations confined to a ragged last tile (edge-leak, edge-stale) fail it exactly where a tile is ragged."""
import os

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


# ---- the tile-geometry sweep (conv_float64.GEOMETRY, edge_shapes): what tests/test_gpu_conv_edges.py runs on the GPU --------------------------

def _edge_ids():
    from tests.test_gpu_conv_float64 import CONFIGS
    # id -> (tag of ROUNDINGS, stride); the split forms of the experiments build carry W4's profile tag and a count of their own
    return {**{cid: (cid if cid in ("W4S", "W4H", "W2S") else c[0], c[1]) for cid, c in CONFIGS.items()}, "HEAD": ("HEAD", 2), "F1": ("F1", 2)}


EDGE_IDS = _edge_ids()
SWEPT = [cid for cid in EDGE_IDS if cid != "HEAD"]          # the head's emulation is two chained convolutions: its own test below


def _edge_alg_tile_n(cid):
    """(emulation algorithm, the tile the edge mutations cut, n) of an id on its first channel configuration"""
    tag = EDGE_IDS[cid][0]
    alg = F.emulation_of(tag)
    cp = 3 if cid == "F1" else F.padded(F.EDGE_CHANNELS[cid][0][0])
    th, tw = F.GEOMETRY[cid][:2]
    if alg in WINO:
        m = F.matrices(alg)[2].shape[0]
        assert (th, tw) == ((1, m) if alg == "1D" else (m, m)), "GEOMETRY[%s]: not the tile of %s" % (cid, alg)
        tile = (th, tw)
    else:
        tile = F.mutation_tile(cid)
    return alg, tile, min(F.n_roundings(tag, cp), F.emulation_n(alg, cp))


def test_geometry_table_names_every_kernel_and_cites_its_source():
    assert set(F.GEOMETRY) == set(EDGE_IDS) == set(F.EDGE_CHANNELS)
    for cid, (th, tw, bh, bw, where) in F.GEOMETRY.items():
        assert 1 <= th <= bh and 1 <= tw <= bw, cid
        name, lines = where.split(":")
        paths = [os.path.join(F.ROOT, d, name) for d in ("back2future_amd/csrc", "tools/experiments/csrc")]
        path = [p for p in paths if os.path.exists(p)]
        assert path, "%s: no %s" % (cid, name)
        with open(path[0]) as f:
            n_lines = len(f.readlines())
        assert all(1 <= int(x) <= n_lines for part in lines.split(",") for x in part.split("-")), (cid, where)
        assert all(1 <= ci <= 40 and co >= 1 for ci, co in F.EDGE_CHANNELS[cid]), cid
    assert {co for _, co in F.EDGE_CHANNELS["W4"]} >= {32, 64, 96}          # a 64-output block, the 32-output form, one launch with both


@pytest.mark.parametrize("cid", sorted(EDGE_IDS))
def test_sweep_covers_every_residue_and_block_edge(cid):
    th, tw, bh, bw, _ = F.GEOMETRY[cid]
    shapes = F.edge_shapes(th, tw, bh, bw)
    assert len(shapes) == len(set(shapes)) and all(h > 0 and w > 0 for h, w in shapes)
    for sizes, t, b in (({h for h, _ in shapes}, th, bh), ({w for _, w in shapes}, tw, bw)):
        assert {s % t for s in sizes} == set(range(t)), "%s: a residue mod %d never runs" % (cid, t)
        assert {s for s in (b - 1, b, b + 1) if s > 0} <= sizes, "%s: one under / on / one over %d" % (cid, b)
        assert any(s > 2 * b for s in sizes), "%s: nothing over two blocks of %d" % (cid, b)
        assert set(range(8, b, 8)) <= sizes, "%s: a multiple of 8 below %d is missing" % (cid, b)
    assert max(h for h, _ in shapes) == 2 * bh + 1 and max(w for _, w in shapes) == 2 * bw + 1          # nothing larger than two footprints
    stride = EDGE_IDS[cid][1]
    inputs = F.edge_inputs(cid, stride)
    assert {(h, w) for _, _, h, w in inputs} == set(shapes)
    for H, W, h, w in inputs:
        assert ((H - 1) // stride + 1, (W - 1) // stride + 1) == (h, w) or cid == "HEAD"
        if cid == "HEAD":
            assert ((H - 1) // 2 + 1, (W - 1) // 2 + 1) == (h, w)
    if stride == 2:
        assert {(H % 2, W % 2) for H, W, _, _ in inputs} == ({(0, 0)} if cid == "F1" else {(0, 0), (1, 1)})


@pytest.mark.parametrize("cid", SWEPT)
def test_emulation_meets_the_bound_on_the_sweep(cid):
    """the reference alone stays inside n u S on every sweep shape (gauss, dc, integers), bit-exact on integers on the dyadic paths"""
    alg, _, n = _edge_alg_tile_n(cid)
    stride = EDGE_IDS[cid][1]
    ci, co = F.EDGE_CHANNELS[cid][0]
    failures, worst = [], 0.0
    for H, W, h, w in F.edge_inputs(cid, stride):
        for family in F.EDGE_FAMILIES:
            r, exact = F.edge_emulation_case(alg, family, ci, co, H, W, stride)
            worst = max(worst, r)
            if not r <= n:
                failures.append("%s %s %s %dx%d: err = %.2f u S, bound n = %d" % (cid, alg, family, H, W, r, n))
            if family == "integers" and alg in ("direct", "direct-b", "F2") and not exact:
                failures.append("%s %s integers %dx%d: not bit-exact" % (cid, alg, H, W))
    print("%-10s %-8s worst err / (u S) = %8.3f (n = %d)" % (cid, alg, worst, n))
    assert not failures, "\n".join(failures)


def test_head_emulation_meets_its_bound_on_the_sweep():
    failures = []
    for H, W, h, w in F.edge_inputs("HEAD", 2):
        for family in F.EDGE_FAMILIES:
            x, w1, b1, w2, b2 = F.head_case(family, H, W)
            got = F.direct32(F.direct32(x, w1, b1, 1, True), w2, b2, 2, True)
            assert got.shape[2:] == (h, w)
            r_bound = F.head_measure(got, x, w1, b1, w2, b2)[2]
            if not r_bound <= 1.0:
                failures.append("head %s %dx%d: the emulation is at %.3f of the bound" % (family, H, W, r_bound))
            if family == "integers":
                t = F.conv64(x, w1, b1, 1, False)
                if t.min() < 0 or not np.array_equal(got, F.round32_leaky(F.conv64(t, w2, b2, 2, False), True)):
                    failures.append("head integers %dx%d: not bit-exact" % (H, W))
    assert not failures, "\n".join(failures)


def _edge_mutation_shows(mutate, cut, H, W, stride):
    """does the mutation change a valid output?  edge-leak at stride 2: only where the input size is odd -- the last output of an even map
    never reads past it"""
    if mutate == "edge-stale":
        return cut[1]
    return (cut[0] and (stride == 1 or H % 2 == 1)) or (cut[1] and (stride == 1 or W % 2 == 1))


@pytest.mark.parametrize("mutate", F.EDGE_MUTATIONS)
@pytest.mark.parametrize("cid", SWEPT)
def test_edge_mutations_turn_the_check_red_only_where_a_tile_is_ragged(cid, mutate):
    """an error confined to a ragged last tile fails the bound on every sweep shape that has one (in that dimension), gauss and dc; where
    no tile is ragged the mutation changes nothing"""
    alg, tile, n = _edge_alg_tile_n(cid)
    stride = EDGE_IDS[cid][1]
    ci, co = F.EDGE_CHANNELS[cid][0]
    failures, red, green = [], 0, 0
    for H, W, h, w in F.edge_inputs(cid, stride):
        shows = _edge_mutation_shows(mutate, F.ragged(h, w, tile), H, W, stride)
        for family in ("gauss", "dc"):
            good = F.edge_emulation_case(alg, family, ci, co, H, W, stride)[0]
            bad = F.edge_emulation_case(alg, family, ci, co, H, W, stride, mutate, tile)[0]
            if shows and not bad > n:
                failures.append("%s %s %s %dx%d: err = %.2f u S passes n = %d" % (cid, mutate, family, H, W, bad, n))
            if not shows and not (bad == good and good <= n):
                failures.append("%s %s %s %dx%d: no ragged tile, yet err = %.2f u S against %.2f" % (cid, mutate, family, H, W, bad, good))
        red, green = red + shows, green + (not shows)
    # (edge-leak at stride 1 has no green shape: the sweep holds every height at a ragged width and every width at a ragged height)
    # and none red on the first layer: it serves even maps only, whose last output never reads past the map)
    assert red > 0 or (mutate == "edge-leak" and cid == "F1"), (cid, mutate, red, green)
    assert green > 0 or (mutate == "edge-leak" and stride == 1), (cid, mutate, red, green)
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


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
