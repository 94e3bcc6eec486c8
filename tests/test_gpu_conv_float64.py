"""GPU: every conv kernel against the float64 restatement of tests/conv_float64.py, on every input family, at every launcher branch.

ops.conv3x3 runs each kernel of kKernels (csrc/b2f_api.hip) under the options that force it, ops.conv_head16 the fused head, ops.layer one
first decoder layer of each level (two K segments, the permuted cin_map) under the settings of tests/test_gpu_in_place.py.  The kernel
that ran is read from the profile row of the call and must be the one the case names.  Per case and family:

  1. |got - conv64| <= bound(tag, Ci_padded, S) elementwise, S the yardstick of the algorithm that computed the output channel; where
     every product is zero (the zero image of `sparse`) the result is exactly the bias through the kernel's LeakyReLU, 0 where that is 0;
  2. the worst err / (u S_direct), and for a Winograd kernel the worst err / (u S_wino) too (on `sparse` S_direct is tiny at single outputs
     and the first figure says little), are at most 2 x the float32 emulation's on the same algorithm and family
     (tests/golden/conv_float64_ratios.json, held to a fresh computation by tests/test_conv_float64_cpu.py); the kernels whose chain starts
     at the bias (D1, D2, the first layer) are held to their own emulation and to 2 sqrt(3) x the plain one (conv_float64.BIAS_FIRST_FACTOR);
  3. `integers`: the direct, F(2x2) and split-bf16 kernels and the head give conv64 bit for bit;
  4. every launcher branch (persistent / one tile, block counts, eight-wave / four-wave, tile groups) gives the bits of the first.

ops.conv_first runs the first layer's kernel (3 -> 16, stride 2, with and without ColorNormalize) on the even maps it serves.  The forms of
the experiments build (wino4_split, wino4_hybrid, wino2_split, the 16 -> 16 layer on the bf16 pipe) run where the library has them.
Known red, experiments build only: W2S (wino2_split) 32 -> 128 17x33 `sparse` measures err / (u S_direct) = 453.65 against 2 x 214.40 of the
fp32 F(2x2) emulation (the fp32 W2 kernel: 371.13); its err / (u S_wino) and the bound hold.  The bar is left as it is.
Run with -s for the table (profiles/r20_conv_float64.txt is that printout)."""
import numpy as np
import pytest

from back2future_amd import back2future, ops, weights as W
from tests import conv_float64 as F
from tests import layer_models as L

pytestmark = pytest.mark.gpu

MARGIN = 2.0
TABLE = {}          # (row label, family) -> [worst err / (u S_direct), sum of means, cases, emulation ratio, n]

W4 = {"wino6": 0, "wino1d": 0, "bf16_conv": 1}
# id: (tag, stride, shapes, options, [options of the other branches: same bits], integers are bit exact)
CONFIGS = {
    "D1": ("D1", 1, F.SMALL, {"bf16_conv": 0}, [], True),
    "D2": ("D2", 2, F.STRIDE2 + F.STRIDE2_RAGGED, {"bf16_conv": 0}, [{"bf16_conv": 0, "s2_tiles_per_block": 2}], True),
    "N2": ("N2", 1, F.FIXED["N2"], {}, [], True),
    "C16": ("C16", 1, F.FIXED["C16"], {"bf16_direct": 0}, [], True),      # (an experiments build runs the layer as B16 otherwise)
    "S16": ("S16", 2, F.FIXED["S16"], {}, [], True),
    "W2": ("W2", 1, F.F2X2, {"op_wino_split": 1, "wino8": 0}, [{"op_wino_split": 1, "wino8": 1}], True),
    "W4": ("W4", 1, F.WIDE, dict(W4, wino4_persistent=0), [dict(W4, wino4_persistent=3), dict(W4, wino4_persistent=1)], False),
    "W6": ("W6", 1, F.WIDE, dict(W4, wino6=1, wino6_min_pixels=0), [dict(W4, wino6=1, wino6_min_pixels=0, wino4_persistent=2)], False),
    "V1-1": ("V1", 1, F.WIDE, dict(W4, wino1d=1), [dict(W4, wino1d=1, wino4_persistent=2)], False),
    "V1-2": ("V1", 1, F.WIDE, dict(W4, wino1d=2), [dict(W4, wino1d=2, wino4_persistent=2)], False),
    "E1": ("E1", 1, F.WIDE, dict(W4, bf16_conv=3, bf16_conv_min_pixels=0), [], True),
    "E1-direct": ("E1", 1, [s for s in F.SMALL if s[1] % 4 == 0], {"bf16_conv": 1}, [], True),      # the direct class on the bf16 pipe
    "E2": ("E2", 2, F.STRIDE2 + F.STRIDE2_RAGGED, {"bf16_conv": 1, "s2_loader": 0}, [], True),
    "L2": ("L2", 2, F.STRIDE2, {"bf16_conv": 1, "s2_loader": 2}, [{"bf16_conv": 1, "s2_loader": 2, "s2_tile_groups": 0},
                                                                  {"bf16_conv": 1, "s2_loader": 2, "wino4_persistent": 2}], True),
}
# python -m back2future_amd.build --experiments (run the suite with B2F_LIB=<that library>); the profile tag of a split launch is W4's
EXPERIMENTS = {
    "W4S": ("W4", 1, F.WIDE, dict(W4, wino4_persistent=3, wino4_split=1), [dict(W4, wino4_persistent=1, wino4_split=1)], False),
    "W4H": ("W4", 1, F.WIDE[2:4], dict(W4, wino4_persistent=5, wino4_hybrid=4), [], False),
    "W2S": ("W4", 1, F.WIDE, dict(W4, wino2_split=1), [], False),
    "B16": ("B16", 1, F.FIXED["C16"], {"bf16_direct": 1}, [], True),
}
CONFIGS.update(EXPERIMENTS)
CASES = [(cid, s) for cid, c in CONFIGS.items() for s in c[2]]
_LAYER_MODELS = {}


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    yield m
    m.close()


@pytest.fixture(scope="module", autouse=True)
def _table_and_models():
    yield
    for m in _LAYER_MODELS.values():
        m.close()
    _LAYER_MODELS.clear()
    print("\n%-14s %-8s %12s %12s %12s %6s" % ("kernel", "family", "worst/(uS)", "mean/(uS)", "emulation", "n"))
    for (label, family), (worst, mean, cases, emu, n) in sorted(TABLE.items(), key=lambda kv: (kv[0][0], F.FAMILIES.index(kv[0][1]))):
        print("%-14s %-8s %12.2f %12.3f %12.2f %6d" % (label, family, worst, mean / cases, emu, n))


def _note(label, family, worst, mean, emu, n):
    row = TABLE.setdefault((label, family), [0.0, 0.0, 0, emu, 0])
    row[0], row[1], row[2], row[3], row[4] = max(row[0], worst), row[1] + mean, row[2] + 1, max(row[3], emu), max(row[4], n)


def _channel_groups(cid, co):
    """[(first, end, algorithm, tag whose n bounds it)] of a case's output channels: a wino1d = 1 launch leaves a last n-block of <= 32
    real outputs to the F(4x4) single-N-tile kernel (choose_kernel, csrc/b2f_api.hip); wino6's 32-output block is F(6x6) too"""
    tag = CONFIGS[cid][0]
    alg = F.ROUNDINGS[tag][0]
    cut = min(co, 64 * (co // 64 + (1 if co % 64 > 32 else 0)))          # the n-blocks of 64 with more than 32 real outputs
    if cid == "V1-1":
        return [g for g in ((0, cut, "1D", "V1"), (cut, co, "F4", "W4")) if g[0] < g[1]]
    if cid in ("W4S", "W4H", "W2S"):                                     # b2f_wino4.hip:1604-1609: the last <= 32 outputs stay on fp32 F(4x4)
        return [g for g in ((0, cut, F.ROUNDINGS[cid][0], cid), (cut, co, "F4", "W4")) if g[0] < g[1]]
    if cid == "B16":
        return [(0, co, "direct", "B16")]
    return [(0, co, alg, tag)]


def _check(got, family, x, w, b, val, Sd, stride, groups, ci_padded, label, what, exact, emu_alg=None):
    """assertions 1 - 3 of the module's docstring on one result; returns the list of failures"""
    fails = []
    if got.shape != val.shape:
        return ["%s: shape %s, expected %s" % (what, got.shape, val.shape)]
    leaky_b = F.round32_leaky(b, True)
    for c0, c1, alg, tag in groups:
        S = Sd[:, c0:c1] if alg == "direct" else F.S_wino(x, w[c0:c1], b[c0:c1], alg)
        g, v = got[:, c0:c1], val[:, c0:c1]
        n = F.n_roundings(tag, ci_padded)
        r_alg, _, _ = F.measure(g, v, S)
        r_direct, mean_direct, worst_abs = F.measure(g, v, Sd[:, c0:c1])
        emu = F.recorded(emu_alg or F.emulation_of(tag), family)
        _note("%s (%s)" % (label, alg) if label in ("V1-1", "W4S", "W4H", "W2S") else label, family, r_direct, mean_direct, emu, n)
        print("%-52s %-8s %-3s err/(u S) = %9.2f (n = %5d)  err/(u S_direct) = %10.2f (emulation %10.2f)  max |err| = %.3g" % (
            what, family, alg, r_alg, n, r_direct, emu, worst_abs))
        if not r_alg <= n:
            fails.append("%s %s: error %.2f u S exceeds the bound n = %d (%s)" % (what, family, r_alg, n, alg))
        quiet = S == np.abs(b[c0:c1]).astype(np.float64)[None, :, None, None]          # every product zero
        if not np.array_equal(g[quiet], np.broadcast_to(leaky_b[None, c0:c1, None, None], g.shape)[quiet]):
            fails.append("%s %s: not exactly the bias where every product is zero" % (what, family))
        if not r_direct <= MARGIN * emu:
            fails.append("%s %s: err / (u S_direct) = %.2f, more than %g x the emulation's %.2f (%s)" % (what, family, r_direct, MARGIN, emu, alg))
        if alg != "direct" and not r_alg <= MARGIN * F.recorded(alg, family, True):
            fails.append("%s %s: err / (u S_wino) = %.3f, more than %g x the emulation's %.3f (%s)" % (what, family, r_alg, MARGIN, F.recorded(alg, family, True), alg))
        if emu_alg is None and F.emulation_of(tag) == "direct-b" and not r_direct <= MARGIN * F.BIAS_FIRST_FACTOR * F.recorded("direct", family):
            fails.append("%s %s: err / (u S_direct) = %.2f, more than %g sqrt(3) x the bias-last emulation's %.2f" % (what, family, r_direct, MARGIN, F.recorded("direct", family)))
    if family == "integers" and exact:
        want = F.round32_leaky(F.conv64(x, w, b, stride, False), True)
        if not np.array_equal(got, want):
            fails.append("%s integers: %d of %d outputs differ from the exact result" % (what, int((got != want).sum()), got.size))
    return fails


def _ran(m, call):
    """(result, tag, padded input channels) from the one conv row the call left in the profile"""
    m.profile_reset()
    out = call()
    rows = [n for n, (ms, cnt) in m.profile_read().items() if cnt > 0 and n.startswith("conv")]
    assert len(rows) == 1, rows
    tag, chans = rows[0][4:].split("_")[:2]
    return out, tag, int(chans.split("to")[0])


def test_every_kernel_of_the_table_has_a_case():
    assert {c[0] for k, c in CONFIGS.items() if k not in EXPERIMENTS} == {"D1", "D2", "N2", "W2", "C16", "S16", "W4", "E1", "E2", "L2", "V1", "W6"}
    assert any(s[0] > 264 for s in CONFIGS["W2"][2])            # the 'W2+' row


@pytest.mark.parametrize("cid,shape", CASES, ids=["%s-%dto%d-%dx%d" % ((cid,) + s) for cid, s in CASES])
def test_kernel_on_every_family(hard, cid, shape):
    tag, stride, _, opts, branches, exact = CONFIGS[cid]
    if cid in EXPERIMENTS and not hard.get_option("experiments"):
        pytest.skip("experiment kernel: not in the product library (python -m back2future_amd.build --experiments; B2F_LIB=back2future_amd/libb2f_exp.so)")
    ci, co = shape[:2]
    groups = _channel_groups(cid, co)
    expect = "W4" if (cid == "V1-1" and groups[0][2] == "F4") else tag
    label = "W2+" if (tag == "W2" and ci > 264) else (tag if cid in ("E1-direct", "V1-2") else cid)
    fails, first = [], {}
    what = "%-5s %3d -> %3d %2dx%2d s%d" % ((cid,) + shape + (stride,))
    with hard.options(**opts):           # (one option change per branch, not per family: some of these options repack the model)
        for family in F.FAMILIES:
            x, w, b, val, Sd = F.reference(family, shape, stride, True)
            got, ran, cp = _ran(hard, lambda: ops.conv3x3(hard, x, w, b, stride, True))
            if ran != expect:
                fails.append("%s %s: ran on %s, the case is meant for %s" % (what, family, ran, expect))
                continue
            assert cp == F.padded(ci)
            first[family] = got
            fails += _check(got, family, x, w, b, val, Sd, stride, groups, cp, label, what, exact)
    for other in branches:
        with hard.options(**other):
            for family, got in first.items():
                x, w, b = F.reference(family, shape, stride, True)[:3]
                again, ran2, _ = _ran(hard, lambda: ops.conv3x3(hard, x, w, b, stride, True))
                if ran2 != expect or not np.array_equal(again, got):
                    fails.append("%s %s: options %s ran %s and give %d other bits" % (what, family, other, ran2, int((again != got).sum())))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("cid,shape", [("D1", (40, 12, 17, 33)), ("W2", (72, 68, 17, 33)), ("W4", (72, 68, 17, 33)), ("W6", (72, 68, 17, 33)),
                                       ("V1-2", (72, 68, 17, 33)), ("E1", (72, 68, 17, 33))])
def test_without_the_activation_a_zero_image_gives_exactly_the_bias(hard, cid, shape):
    """leaky = False on `sparse` and `integers`: exactly b where every product is zero; the bound and, where exact, the bits elsewhere"""
    tag, stride, _, opts, _, exact = CONFIGS[cid]
    fails = []
    for family in ("sparse", "integers"):
        x, w, b = F.reference(family, shape, stride, True)[:3]
        val, Sd = F.conv64(x, w, b, stride, False), F.reference(family, shape, stride, True)[4]
        with hard.options(**opts):
            got, ran, cp = _ran(hard, lambda: ops.conv3x3(hard, x, w, b, stride, False))
        assert ran == tag
        alg = F.ROUNDINGS[tag][0]
        S = Sd if alg == "direct" else F.wino_yardstick(family, shape, alg)
        r_alg = F.measure(got, val, S)[0]
        if not r_alg <= F.n_roundings(tag, cp):
            fails.append("%s %s: error %.2f u S exceeds n = %d" % (cid, family, r_alg, F.n_roundings(tag, cp)))
        quiet = S == np.abs(b).astype(np.float64)[None, :, None, None]
        assert quiet.any() or family == "integers"
        if not np.array_equal(got[quiet], np.broadcast_to(b[None, :, None, None], got.shape)[quiet]):
            fails.append("%s %s: not exactly b where every product is zero" % (cid, family))
        if family == "integers" and exact and not np.array_equal(got, val.astype(np.float32)):
            fails.append("%s integers: %d outputs differ from the exact result" % (cid, int((got != val.astype(np.float32)).sum())))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H,Wd", F.HEAD)
def test_fused_head_on_every_family(hard, H, Wd):
    """ops.conv_head16: conv(16, 16, s1) + LeakyReLU + conv(16, 32, s2) + LeakyReLU in one kernel.  The bound carries the first layer's bound
    through the second (conv_float64.head64); the emulation is two chained float32 direct convolutions; S = the second layer's S_direct on
    the float64 map, its worst per family recorded and held to the bound by the CPU file (conv_float64.head_case, head_emulation_case)."""
    fails = []
    for family in F.FAMILIES:
        x, w1, b1, w2, b2 = F.head_case(family, H, Wd)
        got = ops.conv_head16(hard, x, w1, b1, w2, b2)
        r, mean, r_bound, worst_abs = F.head_measure(got, x, w1, b1, w2, b2)
        r_emu = F.recorded("head", family)
        _note("HEAD", family, r, mean, r_emu, F.n_roundings("HEAD", 16))
        what = "head 16 -> 16 -> 32 %2dx%2d" % (H, Wd)
        print("%-52s %-8s err/bound = %.4f  err/(u S2) = %8.2f (emulation %8.2f)  max |err| = %.3g" % (what, family, r_bound, r, r_emu, worst_abs))
        if not r_bound <= 1.0:
            fails.append("%s %s: error is %.3f of the bound" % (what, family, r_bound))
        if not r <= MARGIN * r_emu:
            fails.append("%s %s: err / (u S2) = %.2f, more than %g x the emulation's %.2f" % (what, family, r, MARGIN, r_emu))
        if family == "integers":
            t = F.conv64(x, w1, b1, 1, False)
            assert t.min() >= 0
            want = F.round32_leaky(F.conv64(t, w2, b2, 2, False), True)
            if not np.array_equal(got, want):
                fails.append("%s integers: %d of %d outputs differ from the exact result" % (what, int((got != want).sum()), got.size))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


LAYER_SETTINGS = {"f4x4": "W4", "f6x6": "W6", "wino1d-2": "V1", "bf16-wide": "E1", "f2x2-split": "W2"}
X_FAMILIES = [f for f in F.FAMILIES if f != "integers"]          # the weights are the model's own (tests/test_gpu_in_place.py's draw)


@pytest.mark.parametrize("level", [3, 4, 5, 6, 7])
def test_first_decoder_layer_on_every_family(level):
    """l<level>.flow.conv1 of the Hard model through ops.layer -- run_conv, two K segments, the permuted cin_map, chunk-planar buffers --
    on the input families (the weights stay the model's), under every setting that names a kernel of the wide stride-1 class"""
    name = L.name("flow", level, 1)
    v = W.views(L.flat("hard"), False)
    wt, b = v[name + ".w"], v[name + ".b"]
    co, ci = wt.shape[:2]
    H, Wd = 17, 33
    fails = []
    for family in X_FAMILIES:
        x = F.make_case(family, F.SEED + level, F.BATCH, ci, 1, H, Wd)[0]
        val, Sd = F.conv64(x, wt, b, 1, True), F.S_direct(x, wt, b, 1)
        for setting, tag in LAYER_SETTINGS.items():
            if setting not in _LAYER_MODELS:
                _LAYER_MODELS[setting] = L.open_model("hard", setting)
            m = _LAYER_MODELS[setting]
            got, ran, cp = _ran(m, lambda: ops.layer(m, "flow", level, 1, x))
            what = "%s %dx%d %-10s" % (name, H, Wd, setting)
            if ran != tag:
                fails.append("%s %s: ran on %s, the setting names %s" % (what, family, ran, tag))
                continue
            alg = F.ROUNDINGS[tag][0]
            fails += _check(got, family, x, wt, b, val, Sd, 1, [(0, co, alg, tag)], cp, "layer " + tag, what, False)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", F.FIRST, ids=lambda s: "%dx%d" % s[2:])
def test_first_layer_on_every_family(hard, shape, normalize):
    """ops.conv_first: conv(3, 16, s2) + LeakyReLU on the three frames as the forward launches it (launch_conv_first), one family draw per frame.
    normalize: ColorNormalize first; the float64 reference normalises in float64 with the kernel's float32 constants, and the two roundings
    per input are in n (ROUNDINGS['F1']); its emulation is recorded apart ('first-norm': no family keeps integer inputs).  The chain starts at
    the bias: the direct-b emulation.  integers without normalize: bit for bit."""
    _, _, H, Wd = shape
    fails = []
    for family in F.FAMILIES:
        x9, w, b, x64 = F.first_case(family, shape, normalize)
        got = ops.conv_first(hard, x9, w, b, normalize)
        val, Sd = F.conv64(x64, w, b, 2, True), F.S_direct(x64, w, b, 2)
        what = "first 3 -> 16 %2dx%2d s2%s" % (H, Wd, " normalized" if normalize else "")
        fails += _check(got, family, x64, w, b, val, Sd, 2, [(0, 16, "direct", "F1")], 3, "F1 norm" if normalize else "F1", what, not normalize,
                        "first-norm" if normalize else None)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)
