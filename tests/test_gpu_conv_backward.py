"""GPU: ops.conv3x3_backward (b2f_op_conv3x3_backward, csrc/b2f_convbwd.hip) against the float64 restatement of
tests/conv_backward_float64.py, batch 2, on every input family, with and without the activation, in both layouts.

  1. gw and gb within (longest_chain + partials + 2) u S, the plan query supplying both counts; gx within the bound of the forward kernel
     that ran (its tag is read from the call's profile row) plus the rounding of g'; gw's worst err / (u S_gw) at most 2 x the float32
     emulation's of the family (tests/golden/conv_backward_ratios.json, held fresh by tests/test_conv_backward_cpu.py);
  2. option op_gradw_partials = 3: the same bounds with a ragged last partial, and the plan query reports 3;
  3. `integers` without the activation: gw, gb and (on a direct or F(2x2) forward kernel) gx equal float64 bit for bit;
  4. two calls give the same bits, and a call for one output alone gives the bits of the full call;
  5. an all-zero gy gives all-zero outputs;  6. an all-zero last image of gy contributes nothing;
  7. one non-zero of gy and one of x meet in exactly one tap of one (co, ci), for each tap, at an interior and at a corner pixel;
  8. the refusals name the argument and write nothing;
  9. every call runs under the OpStage guards: a guard hit is the entry's error and fails the test that made the call.
Run with -s for the figures."""
import ctypes as C

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import conv_backward_float64 as K
from tests import conv_float64 as F

pytestmark = pytest.mark.gpu

MARGIN = 2.0                                    # tests/test_gpu_conv_float64.py: MARGIN
EXACT_TAGS = ("D1", "N2", "C16", "W2", "E1")    # make_case: `integers` is exact on the direct, F(2x2) and split-bf16 paths
SHAPES = K.all_shapes()
_ID = lambda s: "%dto%d-%dx%d" % s


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    yield m
    m.close()


def _run(m, x, w, gy, y, leaky, layout, want=("x", "w", "b")):
    """(outputs, tag of the forward kernel that computed gx or None, profile rows of the call)"""
    m.profile_reset()
    out = ops.conv3x3_backward(m, x, w, gy, y=y, leaky=leaky, layout=layout, want=want)
    rows = sorted(n for n, (ms, cnt) in m.profile_read().items() if cnt > 0)
    conv = [n for n in rows if n.startswith("conv") and not n.startswith("convbwd_")]
    assert len(conv) == (1 if "x" in want else 0), rows
    assert "convbwd_mask" in rows
    assert ("convbwd_gradw" in rows and "convbwd_reduce" in rows) == ("w" in want or "b" in want), rows
    return out, (conv[0][4:].split("_")[0] if conv else None), rows


def _within(got, val, S, n, what):
    """failures of |got - val| <= n u S elementwise; the worst err / (u S)"""
    fails = []
    if got.shape != val.shape:
        return ["%s: shape %s, expected %s" % (what, got.shape, val.shape)], float("inf")
    r = F.measure(got, val, S)[0]
    if not r <= n:
        fails.append("%s: error %.2f u S exceeds the bound n = %d" % (what, r, n))
    if not np.array_equal(got[S == 0], np.zeros_like(got)[S == 0]):
        fails.append("%s: not exactly zero where every product is zero" % what)
    return fails, r


def _check(m, family, shape, leaky, layout, expect_partials=None):
    """checks 1 (and 2) on one call: the list of failures"""
    Ci, Co, H, W = shape
    x, w, y, gy = K.case(family, shape, leaky)
    (gx, gw, gb), (_, Sw, Sb), g = K.reference(family, shape, leaky)
    P, chain = ops.conv3x3_backward_plan(m, K.BATCH, Ci, H, W, Co)
    if expect_partials is not None:
        assert P == expect_partials
    assert 1 <= chain <= K.BATCH * H * W and P >= 1
    out, tag, _ = _run(m, x, w, gy, y, leaky, layout)
    what = "%3d -> %3d %2dx%2d %-8s leaky %d layout %d" % (shape + (family, leaky, layout))
    n = chain + P + 2
    fails, rw = _within(out["w"], gw, Sw, n, what + " gw")
    f2, rb = _within(out["b"], gb, Sb, n, what + " gb")
    fails += f2
    emu = K.recorded_ratios()[family]
    if not rw <= MARGIN * emu:
        fails.append("%s gw: err / (u S_gw) = %.2f, more than %g x the emulation's %.2f" % (what, rw, MARGIN, emu))
    if tag not in F.ROUNDINGS:
        return fails + ["%s gx: unknown forward kernel %r" % (what, tag)]
    wt = K.rotated(w.astype(np.float64))
    zero = np.zeros(Ci)
    S_round = F.S_direct(g, wt, zero)
    alg = F.ROUNDINGS[tag][0]
    S_alg = S_round if alg == "direct" else F.yardstick(alg, g, wt, zero)
    bound = K.bound_gx(tag, Co, S_alg, S_round)
    f3, rx = _within(out["x"], gx, bound / K.U, 1, what + " gx (%s, in units of its bound)" % tag)
    fails += f3
    print("%s  P %d chain %4d  gw %7.2f u S (emulation %6.2f)  gb %7.2f u S  gx %s %.3f of its bound" % (what, P, chain, rw, emu, rb, tag, rx))
    return fails


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_bounds_on_every_family(hard, shape, family):
    """check 1"""
    fails = []
    for leaky in (False, True):
        for layout in (0, 1):
            fails += _check(hard, family, shape, leaky, layout)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("shape", K.FORCED, ids=_ID)
def test_three_forced_partials(hard, shape):
    """check 2: 36 strips as 12 + 12 + 12, whose partials begin in the middle of an image, and 28 strips as 10 + 10 + 8: a shorter last one"""
    fails = []
    with hard.options(op_gradw_partials=3):
        for family in F.FAMILIES:
            for layout in (0, 1):
                fails += _check(hard, family, shape, True, layout, expect_partials=3)
    assert hard.get_option("op_gradw_partials") == 0
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_integers_are_bit_exact(hard, shape):
    """check 3"""
    x, w, _, gy = K.case("integers", shape, False)
    (gx, gw, gb), _, _ = K.reference("integers", shape, False)
    for layout in (0, 1):
        out, tag, _ = _run(hard, x, w, gy, None, False, layout)
        assert np.array_equal(out["w"].astype(np.float64), gw), "gw: %d of %d differ" % ((out["w"] != gw).sum(), gw.size)
        assert np.array_equal(out["b"].astype(np.float64), gb)
        if tag in EXACT_TAGS:
            assert np.array_equal(out["x"].astype(np.float64), gx), "gx on %s: %d of %d differ" % (tag, (out["x"] != gx).sum(), gx.size)


@pytest.mark.parametrize("shape", [(40, 36, 17, 33), (200, 96, 13, 49)], ids=_ID)
def test_same_bits_again_and_alone(hard, shape):
    """check 4"""
    x, w, y, gy = K.case("gauss", shape, True)
    for layout in (0, 1):
        full, _, _ = _run(hard, x, w, gy, y, True, layout)
        again, _, _ = _run(hard, x, w, gy, y, True, layout)
        for k in "xwb":
            assert np.array_equal(full[k], again[k]), k
            alone, _, _ = _run(hard, x, w, gy, y, True, layout, want=(k,))
            assert set(alone) == {k} and np.array_equal(alone[k], full[k]), k


def test_zero_gradient_gives_zeros(hard):
    """check 5"""
    shape = (40, 36, 17, 33)
    x, w, y, gy = K.case("gauss", shape, True)
    for leaky in (False, True):
        for layout in (0, 1):
            out, _, _ = _run(hard, x, w, np.zeros_like(gy), y if leaky else None, leaky, layout)
            for k in "xwb":
                assert not out[k].any(), k


@pytest.mark.parametrize("shape", [(40, 36, 17, 33), (72, 68, 13, 49)], ids=_ID)
def test_a_zero_last_image_contributes_nothing(hard, shape):
    """check 6: gy of the last image all zero (x there is not): gw, gb and gx of image 0 are the one-image call's, gx of the last image is
    zero.  With one partial both calls add image 0's pixels in one chain, and the zeros behind it change no bit; under the rule the two
    batch sizes are cut into partials at different pixels, and the sums agree to the bound only."""
    x, w, y, gy = K.case("gauss", shape, True)
    gy = gy.copy()
    gy[-1] = 0
    for layout in (0, 1):
        with hard.options(op_gradw_partials=1):
            two, _, _ = _run(hard, x, w, gy, y, True, layout)
            one, _, _ = _run(hard, x[:-1], w, gy[:-1], y[:-1], True, layout)
        assert np.array_equal(two["w"], one["w"]) and np.array_equal(two["b"], one["b"])
        assert np.array_equal(two["x"][:-1], one["x"]) and not two["x"][-1].any()
        ruled, _, _ = _run(hard, x, w, gy, y, True, layout, want=("w",))
        (_, gw, _), (_, Sw, _), _ = K.reference("gauss", shape, True)
        P, chain = ops.conv3x3_backward_plan(hard, K.BATCH, shape[0], shape[2], shape[3], shape[1])
        assert np.all(np.abs(ruled["w"].astype(np.float64) - one["w"]) <= 2 * K.bound_gw(chain, P, Sw))


@pytest.mark.parametrize("corner", [False, True], ids=["interior", "corner"])
def test_one_tap_of_one_channel_pair(hard, corner):
    """check 7: 40 -> 36 channels on a 5 x 35 map (three row bands, two column strips); gy = 3 at (image 1, co 29, one pixel), x = 5 at
    (image 1, ci 13, the pixel tap (ky, kx) reads for it): gw is 15 at [29, 13, ky, kx] and zero elsewhere, gb is 3 at 29.  corner: gy's
    pixel is the corner of the map from which the tap still points inside."""
    Ci, Co, H, W = 40, 36, 5, 35
    for ky in range(3):
        for kx in range(3):
            oy, ox = ((0 if ky >= 1 else H - 1), (0 if kx >= 1 else W - 1)) if corner else (2, 32)
            gy = np.zeros((2, Co, H, W), np.float32)
            x = np.zeros((2, Ci, H, W), np.float32)
            gy[1, 29, oy, ox] = 3
            x[1, 13, oy + ky - 1, ox + kx - 1] = 5
            w = np.zeros((Co, Ci, 3, 3), np.float32)
            want_w = np.zeros_like(w)
            want_w[29, 13, ky, kx] = 15
            want_b = np.zeros(Co, np.float32)
            want_b[29] = 3
            for layout in (0, 1):
                out, _, _ = _run(hard, x, w, gy, None, False, layout, want=("w", "b"))
                assert np.array_equal(out["w"], want_w), (ky, kx, layout, np.argwhere(out["w"] != want_w)[:4])
                assert np.array_equal(out["b"], want_b), (ky, kx, layout)


def test_refusals(hard):
    """check 8"""
    B, Ci, Co, H, W = 2, 8, 8, 4, 4
    x, w = np.ones((B, Ci, H, W), np.float32), np.ones((Co, Ci, 3, 3), np.float32)
    y = gy = np.ones((B, Co, H, W), np.float32)
    sentinel = np.float32(-7.5)
    outs = [np.full_like(x, sentinel), np.full_like(w, sentinel), np.full(Co, sentinel)]
    p = _lib.fptr

    def call(x_=p(x), B_=B, Ci_=Ci, H_=H, W_=W, w_=p(w), Co_=Co, stride=1, leaky=1, y_=p(y), gy_=p(gy), layout=0, o=(0, 1, 2)):
        ptr = [p(outs[i]) if i in o else None for i in range(3)]
        return _lib.lib().b2f_op_conv3x3_backward(hard._h, x_, B_, Ci_, H_, W_, w_, Co_, stride, leaky, y_, gy_, layout, *ptr)

    cases = [(dict(x_=None), "x is null"), (dict(w_=None), "w is null"), (dict(gy_=None), "grad_y is null"), (dict(y_=None), "y is null"),
             (dict(o=()), "grad_x, grad_w and grad_b are all null"), (dict(stride=2), "stride"), (dict(stride=0), "stride"),
             (dict(layout=2), "layout"), (dict(B_=0), "B must be positive"), (dict(Ci_=0), "Ci must be positive"),
             (dict(H_=-1), "H must be positive"), (dict(W_=0), "W must be positive"), (dict(Co_=0), "Co must be positive")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        msg = _lib.lib().b2f_last_error().decode()
        assert msg.startswith("b2f_op_conv3x3_backward: ") and text in msg, (kw, msg)
        assert all((o == sentinel).all() for o in outs), kw
    assert call(y_=None, leaky=0) == 0 and not any((o == sentinel).any() for o in outs)          # y is not needed without the activation
    with pytest.raises(_lib.B2FError, match="stride must be 1"):
        ops.conv3x3_backward(hard, x, w, gy, y=y, leaky=True, stride=2)
    parts, chain = C.c_int(), C.c_longlong()
    assert _lib.lib().b2f_op_conv3x3_backward_plan(hard._h, B, Ci, 0, W, Co, C.byref(parts), C.byref(chain)) != 0
    assert "H must be positive" in _lib.lib().b2f_last_error().decode()
    assert ops.conv3x3_backward_plan(hard, B, Ci, H, W, Co) == (1, B * H * W)
