"""The float64 restatement of the warp + cost volume (tests/cv_float64.py) and the fp32 oracle hold each other: the oracle's composition
(warping_unit x2 + costvol x2, as test_warp_costvol_fused composes it) meets the derived bar (C + 16) * 2^-24 * S against the restatement
on the shapes the GPU test runs, and the restatement itself gives known answers.  Run with -s for the worst ratio per shape.

Every shape runs under all three flows; the two largest maps are cut to a quarter.  Measured: the worst ratio err / (2^-24 S) is 5.9 (bounds
24 .. 208), the largest absolute error 3.4e-7."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import cv_float64 as F

N_CU = 256      # the shape list of an MI355X in SPX mode; the GPU test builds its own from the device's count
SHAPES = F.shapes(N_CU)
# the oracle and the restatement of the two largest shapes take seconds: a quarter of each is the same check (the issue allows it)
QUARTER = {"full-round": (1, 128, 240), "full-round-c8": (1, 128, 240)}


def _oracle(maps, flow, k, win=9):
    ref, f3, f1 = maps
    w3 = O.warping_unit(f3, flow, k) if flow is not None else f3
    w1 = O.warping_unit(f1, flow, -k) if flow is not None else f1
    return np.concatenate([O.costvol([ref, w3], win, True), O.costvol([ref, w1], win, False)], 1)


def _cases():
    for name, C, B, h, w, k, branch in SHAPES:
        if name in QUARTER:
            B, h, w = QUARTER[name]
        for kind in F.FLOW_KINDS:
            yield pytest.param(name, C, B, h, w, k, kind, id="%s-%s" % (name, kind))


@pytest.mark.parametrize("name,C,B,h,w,k,kind", list(_cases()))
def test_oracle_meets_the_bar(name, C, B, h, w, k, kind):
    seed = C * 1009 + h * 31 + w
    maps = F.make_maps(seed, B, C, h, w)
    flow = F.make_flow(kind, seed + 1, B, h, w, k)
    val, S = F.warp_costvol64(*maps, flow, k)
    F.check(_oracle(maps, flow, k), val, S, C, "oracle %-16s C %3d %dx%dx%d k %g %s" % (name, C, B, h, w, k, kind))


@pytest.mark.parametrize("name", ["bits-wide", "bits-tall"])
def test_translation_crosses_the_coordinate_fields(name, kind="translation"):
    """The 12-bit tap-coordinate fields of the unit kernels' sampling records: on the 4096 maps the translation flow puts left / top taps on both sides of
    255|256, 1023|1024, 2047|2048 with a blend across each boundary, and uses coordinate 4095 both as a left tap without a right neighbour and as
    the right neighbour of 4094 -- in either direction (+k future, -k past)"""
    C, B, h, w, k, branch = {s[0]: s[1:] for s in SHAPES}[name]
    axis, size = (0, w) if name == "bits-wide" else (1, h)
    assert size == 4096
    flow = F.make_flow(kind, C * 1009 + h * 31 + w + 1, B, h, w, k)              # the flow of test_oracle_meets_the_bar and of the GPU test
    for kk in (k, -k):
        pt, wt = F.tap_index(flow, kk, axis, size)
        assert {255, 256, 1023, 1024, 2047, 2048, 4095} <= set(np.unique(pt).tolist())
        for edge in (255, 1023, 2047, 4094):
            assert np.any((pt == edge) & (wt < 1)), "no blend across %d|%d" % (edge, edge + 1)
        assert np.any(pt == 4095)


@pytest.mark.parametrize("n_cu", [16, 32, 64, 80, 128, 256, 304])
def test_shapes_reach_their_branches(n_cu):
    """the shape list is built from the CU count: at every count each shape of the automatic rule reaches the branch it names"""
    for name, C, B, h, w, k, branch in F.shapes(n_cu):
        if branch is not None:
            assert F.auto_variant(n_cu, B, (C + 7) // 8 * 8, h, w) == F.BRANCH_VARIANT(branch), (n_cu, name)


def test_moving_impulse():
    """CostVolMulti.lua:225-254: a point moving (+1, +1) per frame lights channel (-1 + 4) * 9 + (-1 + 4) in both volumes"""
    h = w = 16
    prev = np.zeros((1, 8, h, w), np.float32); cur = prev.copy(); nxt = prev.copy()
    prev[0, 0, 4, 5] = 8; cur[0, 0, 5, 6] = 1; nxt[0, 0, 6, 7] = 8
    cv, S = F.warp_costvol64(cur, nxt, prev, None, 0.0)
    c = 3 * 9 + 3
    assert cv[0, c, 5, 6] == 1 and cv[0, 81 + c, 5, 6] == 1
    assert cv[0, :81].sum() == 1 and cv[0, 81:].sum() == 1
    np.testing.assert_array_equal(S, cv)


def test_zero_flow_is_no_warp():
    maps = F.make_maps(5, 2, 8, 7, 9)
    a = F.warp_costvol64(*maps, np.zeros((2, 2, 7, 9), np.float32), 2.5)
    b = F.warp_costvol64(*maps, None, 2.5)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    # and the unwarped cost volume written out for one element of each direction: d = (qx + 4) * 9 + (qy + 4)
    ref, fut, past = [m.astype(np.float64) for m in maps]
    qx, qy, y, x = 2, -3, 3, 5
    d = (qx + 4) * 9 + (qy + 4)
    assert np.isclose(b[0][1, d, y, x], (ref[1, :, y, x] * fut[1, :, y - qy, x - qx]).sum() / 8, rtol=1e-14, atol=0)
    assert np.isclose(b[0][1, 81 + d, y, x], (ref[1, :, y, x] * past[1, :, y + qy, x + qx]).sum() / 8, rtol=1e-14, atol=0)
    assert b[0][1, (-4 + 4) * 9 + 4, y, 8] == 0 and b[0][1, 81 + (4 + 4) * 9 + 4, y, 8] == 0      # qx -4 forward, +4 backward: column x + 4 is outside the map


def test_one_pixel_flow_is_a_shift():
    """k * flow = (+1, 0): the future map is read one column to the right, the past map one column to the left, the border column clamped"""
    maps = F.make_maps(6, 2, 8, 6, 11)
    ref, fut, past = maps
    flow = np.zeros((2, 2, 6, 11), np.float32)
    flow[:, 0] = 1.0
    got, gS = F.warp_costvol64(ref, fut, past, flow, 1.0)
    idx = np.arange(11)
    fs, ps = fut[..., np.minimum(idx + 1, 10)], past[..., np.maximum(idx - 1, 0)]
    vf, sf = F.costvol64(ref, fs, 9, True)
    vb, sb = F.costvol64(ref, ps, 9, False)
    np.testing.assert_array_equal(got, np.concatenate([vf, vb], 1))
    np.testing.assert_array_equal(gS, np.concatenate([sf, sb], 1))


@pytest.mark.parametrize("C,B,h,w", [(6, 2, 11, 13), (8, 1, 1, 2)])
@pytest.mark.parametrize("win", [3, 5, 7, 11])
def test_generic_windows(win, C, B, h, w):
    r = np.random.default_rng(win * 100 + C)
    ref = r.standard_normal((B, C, h, w), dtype=np.float32)
    frm = r.standard_normal((B, C, h, w), dtype=np.float32)
    for fwd in (True, False):
        val, S = F.costvol64(ref, frm, win, fwd)
        assert val.shape == (B, win * win, h, w)
        F.check(O.costvol([ref, frm], win, fwd), val, S, C, "oracle costvol win %2d %s C %d %dx%dx%d" % (win, "fwd" if fwd else "bwd", C, B, h, w))
