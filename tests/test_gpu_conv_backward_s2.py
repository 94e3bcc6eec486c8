"""GPU: ops.conv3x3s2_backward (b2f_op_conv3x3s2_backward, csrc/b2f_convbwd.hip) against the float64 restatement of
tests/conv_backward_s2_float64.py, batch 2, on every input family, with and without the activation, in both layouts.

  1. gw and gb within (longest_chain + partials + 2) u S, the plan query supplying both counts; gx within (taps * padded(Co) + 2) u S_gx
     elementwise; gw's and gx's worst err / (u S) at most 2 x the float32 emulation's of the family
     (tests/golden/conv_backward_s2_ratios.json, held fresh by tests/test_conv_backward_s2_cpu.py);
  2. option op_gradw_partials = 3: the same bounds with a ragged last partial, and the plan query reports 3;
  3. `integers` without the activation: gw, gb and gx equal float64 bit for bit;
  4. two calls give the same bits, and a call for one output alone gives the bits of the full call;
  5. an all-zero gy gives all-zero outputs;  6. an all-zero last image of gy contributes nothing;
  7. one non-zero of gy meets one of x in exactly one tap of one (co, ci), and one of w at exactly one pixel of gx (or none, outside the
     map), for each tap, at an interior pixel and at each corner, on an odd and on an even map;
  8. the refusals name the argument and write nothing;
  9. every call runs under the OpStage guards: a guard hit is the entry's error and fails the test that made the call.
Run with -s for the figures."""
import ctypes as C

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import conv_backward_s2_float64 as K
from tests import conv_float64 as F

pytestmark = pytest.mark.gpu

MARGIN = 2.0                                    # tests/test_gpu_conv_float64.py: MARGIN
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
    """(outputs, profile rows of the call)"""
    m.profile_reset()
    out = ops.conv3x3s2_backward(m, x, w, gy, y=y, leaky=leaky, layout=layout, want=want)
    rows = sorted(n for n, (ms, cnt) in m.profile_read().items() if cnt > 0)
    assert "convbwd_mask" in rows
    assert ("convbwd_gradx_s2" in rows) == ("x" in want), rows
    assert not [n for n in rows if n.startswith("conv") and not n.startswith("convbwd_")], rows          # no forward kernel runs
    assert ("convbwd_gradw" in rows and "convbwd_reduce" in rows) == ("w" in want or "b" in want), rows
    return out, rows


def _within(got, val, S, n, what):
    """failures of |got - val| <= n u S elementwise (n a number or an array); the worst err / (u S)"""
    fails = []
    if got.shape != val.shape:
        return ["%s: shape %s, expected %s" % (what, got.shape, val.shape)], float("inf")
    r = F.measure(got, val, S)[0]
    if not F.measure(got, val, S * n)[0] <= 1.0:
        fails.append("%s: error %.2f u S exceeds the bound n = %s" % (what, r, np.max(n)))
    if not np.array_equal(got[S == 0], np.zeros_like(got)[S == 0]):
        fails.append("%s: not exactly zero where every product is zero" % what)
    return fails, r


def _check(m, family, shape, leaky, layout, expect_partials=None):
    """checks 1 (and 2) on one call: the list of failures"""
    Ci, Co, H, W = shape
    x, w, y, gy = K.case(family, shape, leaky)
    (gx, gw, gb), (Sx, Sw, Sb), _ = K.reference(family, shape, leaky)
    P, chain = ops.conv3x3s2_backward_plan(m, K.BATCH, Ci, H, W, Co)
    if expect_partials is not None:
        assert P == expect_partials
    assert 1 <= chain <= K.BATCH * gy.shape[2] * gy.shape[3] and P >= 1
    out, _ = _run(m, x, w, gy, y, leaky, layout)
    what = "%3d -> %3d %2dx%2d %-8s leaky %d layout %d" % (shape + (family, leaky, layout))
    n = chain + P + 2
    fails, rw = _within(out["w"], gw, Sw, n, what + " gw")
    f2, rb = _within(out["b"], gb, Sb, n, what + " gb")
    f3, rx = _within(out["x"], gx, Sx, np.broadcast_to(K.gx_roundings(Co, H, W)[None, None], Sx.shape), what + " gx")
    fails += f2 + f3
    rec = K.recorded_ratios()
    for name, r in (("gw", rw), ("gx", rx)):
        emu = rec[name][family]
        if not r <= MARGIN * emu:
            fails.append("%s %s: err / (u S) = %.2f, more than %g x the emulation's %.2f" % (what, name, r, MARGIN, emu))
    print("%s  P %d chain %4d  gw %7.2f u S (emulation %6.2f)  gb %7.2f u S  gx %7.2f u S (emulation %6.2f)"
          % (what, P, chain, rw, rec["gw"][family], rb, rx, rec["gx"][family]))
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
    """check 2: 20 strips as 7 + 7 + 6 and 16 strips as 6 + 6 + 4, a shorter last partial; the partials begin in the middle of an image"""
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
        out, _ = _run(hard, x, w, gy, None, False, layout)
        assert np.array_equal(out["w"].astype(np.float64), gw), "gw: %d of %d differ" % ((out["w"] != gw).sum(), gw.size)
        assert np.array_equal(out["b"].astype(np.float64), gb)
        assert np.array_equal(out["x"].astype(np.float64), gx), "gx: %d of %d differ" % ((out["x"] != gx).sum(), gx.size)


@pytest.mark.parametrize("shape", [(40, 36, 17, 34), (64, 96, 13, 49)], ids=_ID)
def test_same_bits_again_and_alone(hard, shape):
    """check 4"""
    x, w, y, gy = K.case("gauss", shape, True)
    for layout in (0, 1):
        full, _ = _run(hard, x, w, gy, y, True, layout)
        again, _ = _run(hard, x, w, gy, y, True, layout)
        for k in "xwb":
            assert np.array_equal(full[k], again[k]), k
            alone, _ = _run(hard, x, w, gy, y, True, layout, want=(k,))
            assert set(alone) == {k} and np.array_equal(alone[k], full[k]), k


def test_zero_gradient_gives_zeros(hard):
    """check 5"""
    shape = (40, 36, 17, 34)
    x, w, y, gy = K.case("gauss", shape, True)
    for leaky in (False, True):
        for layout in (0, 1):
            out, _ = _run(hard, x, w, np.zeros_like(gy), y if leaky else None, leaky, layout)
            for k in "xwb":
                assert not out[k].any(), k


@pytest.mark.parametrize("shape", [(40, 36, 17, 34), (64, 96, 13, 49)], ids=_ID)
def test_a_zero_last_image_contributes_nothing(hard, shape):
    """check 6: gy of the last image all zero (x there is not): with one partial gw, gb and gx of image 0 are the one-image call's bit for
    bit (both calls add image 0's pixels in one chain, and the zeros behind it change no bit), and gx of the last image is zero"""
    x, w, y, gy = K.case("gauss", shape, True)
    gy = gy.copy()
    gy[-1] = 0
    for layout in (0, 1):
        with hard.options(op_gradw_partials=1):
            two, _ = _run(hard, x, w, gy, y, True, layout)
            one, _ = _run(hard, x[:-1], w, gy[:-1], y[:-1], True, layout)
        assert np.array_equal(two["w"], one["w"]) and np.array_equal(two["b"], one["b"])
        assert np.array_equal(two["x"][:-1], one["x"]) and not two["x"][-1].any()


@pytest.mark.parametrize("where", ["interior", "top-left", "top-right", "bottom-left", "bottom-right"])
@pytest.mark.parametrize("H,W", [(5, 35), (6, 36)], ids=["5x35", "6x36"])
def test_one_tap_of_one_channel_pair(hard, H, W, where):
    """check 7: 40 -> 36 channels; gy = 3 at (image 1, co 29, one output pixel).  x = 5 at (image 1, ci 13, the pixel tap (ky, kx) reads for
    it), if the map has it: gw is 15 at [29, 13, ky, kx] and zero elsewhere, gb is 3 at 29.  w = 5 at [29, 13, ky, kx]: gx is 15 at (image
    1, ci 13, (2 oy + ky - 1, 2 ox + kx - 1)) and zero elsewhere, all zero if that pixel is outside the map."""
    Ci, Co = 40, 36
    Ho, Wo = K.out_size(H), K.out_size(W)
    oy, ox = {"interior": (1, 16), "top-left": (0, 0), "top-right": (0, Wo - 1), "bottom-left": (Ho - 1, 0), "bottom-right": (Ho - 1, Wo - 1)}[where]
    for ky in range(3):
        for kx in range(3):
            iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
            inside = 0 <= iy < H and 0 <= ix < W
            gy = np.zeros((2, Co, Ho, Wo), np.float32)
            gy[1, 29, oy, ox] = 3
            x = np.zeros((2, Ci, H, W), np.float32)
            w = np.zeros((Co, Ci, 3, 3), np.float32)
            w[29, 13, ky, kx] = 5
            want_w, want_x = np.zeros_like(w), np.zeros_like(x)
            if inside:
                x[1, 13, iy, ix] = 5
                want_w[29, 13, ky, kx] = 15
                want_x[1, 13, iy, ix] = 15
            want_b = np.zeros(Co, np.float32)
            want_b[29] = 3
            for layout in (0, 1):
                out, _ = _run(hard, x, w, gy, None, False, layout)
                assert np.array_equal(out["w"], want_w), (ky, kx, layout, np.argwhere(out["w"] != want_w)[:4])
                assert np.array_equal(out["b"], want_b), (ky, kx, layout)
                assert np.array_equal(out["x"], want_x), (ky, kx, layout, np.argwhere(out["x"] != want_x)[:4])


def test_refusals(hard):
    """check 8"""
    B, Ci, Co, H, W = 2, 8, 8, 5, 4
    Ho, Wo = K.out_size(H), K.out_size(W)
    x, w = np.ones((B, Ci, H, W), np.float32), np.ones((Co, Ci, 3, 3), np.float32)
    y = gy = np.ones((B, Co, Ho, Wo), np.float32)
    sentinel = np.float32(-7.5)
    outs = [np.full_like(x, sentinel), np.full_like(w, sentinel), np.full(Co, sentinel)]
    p = _lib.fptr

    def call(x_=p(x), B_=B, Ci_=Ci, H_=H, W_=W, w_=p(w), Co_=Co, leaky=1, y_=p(y), gy_=p(gy), layout=0, o=(0, 1, 2)):
        ptr = [p(outs[i]) if i in o else None for i in range(3)]
        return _lib.lib().b2f_op_conv3x3s2_backward(hard._h, x_, B_, Ci_, H_, W_, w_, Co_, leaky, y_, gy_, layout, *ptr)

    cases = [(dict(x_=None), "x is null"), (dict(w_=None), "w is null"), (dict(gy_=None), "grad_y is null"), (dict(y_=None), "y is null"),
             (dict(o=()), "grad_x, grad_w and grad_b are all null"), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
             (dict(B_=0), "B must be positive"), (dict(Ci_=0), "Ci must be positive"), (dict(H_=-1), "H must be positive"),
             (dict(W_=0), "W must be positive"), (dict(Co_=0), "Co must be positive"), (dict(H_=1 << 13, W_=1 << 13), "too large")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        msg = _lib.lib().b2f_last_error().decode()
        assert msg.startswith("b2f_op_conv3x3s2_backward: ") and text in msg, (kw, msg)
        assert all((o == sentinel).all() for o in outs), kw
    assert call(y_=None, leaky=0) == 0 and not any((o == sentinel).any() for o in outs)          # y is not needed without the activation
    with pytest.raises(ValueError, match="stride-2 layer"):
        ops.conv3x3s2_backward(hard, x, w, np.ones((B, Co, H, W), np.float32))
    parts, chain = C.c_int(), C.c_longlong()
    assert _lib.lib().b2f_op_conv3x3s2_backward_plan(hard._h, B, Ci, 0, W, Co, C.byref(parts), C.byref(chain)) != 0
    msg = _lib.lib().b2f_last_error().decode()
    assert msg.startswith("b2f_op_conv3x3s2_backward_plan: ") and "H must be positive" in msg
    assert ops.conv3x3s2_backward_plan(hard, B, Ci, H, W, Co) == (1, B * Ho * Wo)
