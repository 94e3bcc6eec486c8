"""No GPU: the yardstick of the stride-2 conv layer's backward pass (tests/conv_backward_s2_float64.py) against torch.autograd, the float32
emulations of the gradWeight split and of conv3x3s2_gradx's chain against their bounds and the recorded ratios, the mutations the bounds must
catch, and the C ABI's two new entries."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from back2future_amd import _lib
from tests import conv_backward_float64 as K1
from tests import conv_backward_s2_float64 as K
from tests import conv_float64 as F

ROOT = F.ROOT
ENTRIES = ("b2f_op_conv3x3s2_backward", "b2f_op_conv3x3s2_backward_plan")
_ID = lambda s: "%dto%d-%dx%d" % s


def _autograd(x, w, b, gy, leaky):
    """(y, gx, gw, gb) of conv2d(stride 2, padding 1) + leaky_relu(0.2) in float64"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    xt, wt, bt = t(x).requires_grad_(), t(w).requires_grad_(), t(b).requires_grad_()
    y = torch.nn.functional.conv2d(xt, wt, bt, stride=2, padding=1)
    if leaky:
        y = torch.nn.functional.leaky_relu(y, 0.2)
    y.backward(t(gy))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("leaky", [False, True])
def test_backward64_is_autograd(family, leaky):
    """(a) to 1e-12 of the largest magnitude, at odd and even maps and the smallest ones.  The saved output is autograd's own float64 y, so
    the mask is the same wherever y != 0; the elements forced to y == 0 are compared after forcing the slope by hand."""
    for Ci, Co, H, W in [(40, 36, 17, 33), (40, 36, 18, 64), (40, 36, 9, 34), (8, 8, 1, 1), (8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 5, 8)]:
        Ho, Wo = K.out_size(H), K.out_size(W)
        x, w, b = F.make_case(family, K.SEED, K.BATCH, Ci, Co, H, W)
        gy = F.make_case(family, K.SEED + 1, K.BATCH, Co, Ci, Ho, Wo)[0].astype(np.float64)
        y, gx, gw, gb = _autograd(x, w, b, gy, leaky)
        assert y.shape == gy.shape
        for got, want in zip(K.backward64(x, w, y, gy, leaky), (gx, gw, gb)):
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
        if not leaky:
            continue
        zero = np.random.default_rng(5).random(y.shape) < 0.25
        y0 = np.where(zero, 0.0, y)
        g_forced = np.where(y0 > 0, gy, 0.2 * gy)          # by hand: where y was positive and is now 0, the slope replaces the 1
        if (H, W) == (17, 33):          # the forcing changes something: on the small maps `sparse` may leave gy all zero
            assert (g_forced != np.where(y > 0, gy, 0.2 * gy)).any()
        want = _autograd(x, w, np.zeros(Co), g_forced, False)[1:]
        for got, ref in zip(K.backward64(x, w, y0, gy, True), want):
            assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)


def test_the_shapes_cover_the_kernels_edges():
    """the edge maps are read from the source's constants: output sizes under, on and over both kernels' strips, from odd and even inputs"""
    k = K.kernel_constants()
    assert {"kGradwBandRows", "kGradwS2StripCols", "kGradxS2Rows", "kGradxS2Cols", "kGradxS2Co"} <= set(k)
    outs = {(K.out_size(h), K.out_size(w)) for _, _, h, w in K.all_shapes()[len(K.SHAPES):]}
    for rows, cols in ((k["kGradwBandRows"], k["kGradwS2StripCols"]), (k["kGradxS2Rows"], k["kGradxS2Cols"])):
        assert {(max(rows - 1, 1), cols - 1), (rows, cols), (rows + 1, cols + 1)} <= outs
    assert any(h % 2 and w % 2 for _, _, h, w in K.all_shapes()) and any(h % 2 == 0 and w % 2 == 0 for _, _, h, w in K.all_shapes())
    assert any(co > k["kGradxS2Co"] for _, co, _, _ in K.all_shapes())          # more than one stage of output channels


@pytest.mark.parametrize("shape", K.all_shapes(), ids=_ID)
def test_emulations_stay_within_their_bounds(shape):
    """(b) gradw32 at stride 2 within bound_gw (gb too) for P in {1, 3}, gradx_s2_32 within bound_gx, on every family"""
    for family in F.FAMILIES:
        for P in (1, 3):
            rw, rw_bound, rb, rb_bound = K.gradw_emulation_case(family, shape, P)
            assert rw_bound <= 1.0 and rb_bound <= 1.0, (family, P, rw, rw_bound, rb, rb_bound)
        rx, rx_bound = K.gradx_emulation_case(family, shape)
        assert rx_bound <= 1.0, (family, rx, rx_bound)


def test_stride_one_of_the_emulation_is_the_stride_one_emulation():
    """gradw32's stride argument: at stride 1 it is tests/conv_backward_float64.py's gradw32 bit for bit"""
    x, w, y, gy = K1.case("gauss", (40, 36, 8, 16), True)
    g = K1.masked32(gy, y, True)
    for P in (1, 3):
        for got, want in zip(K.gradw32(x, g, P, 1), K1.gradw32(x, g, P)):
            assert np.array_equal(got, want)


def test_recorded_ratios_are_fresh():
    """(b) tests/golden/conv_backward_s2_ratios.json is what `python -m tests.conv_backward_s2_float64` writes now"""
    fresh, rec = K.compute_ratios(), K.recorded_ratios()
    assert set(fresh) == set(rec) == {"gw", "gx"}
    for what in ("gw", "gx"):
        assert set(fresh[what]) == set(rec[what]) == set(F.FAMILIES)
        for fam in F.FAMILIES:          # the tolerance of tests/test_conv_float64_cpu.py: the float64 sums are BLAS's, whose order is the machine's
            assert abs(fresh[what][fam] - rec[what][fam]) <= 1e-3 * rec[what][fam] + 1e-6, (what, fam, fresh[what][fam], rec[what][fam])
    assert json.load(open(K.RATIOS_PATH)) == rec


@pytest.mark.parametrize("mutate", K.GX_MUTATIONS)
def test_gradx_mutations_break_the_bound(mutate):
    """(c) on gauss each misses gx's bound by more than 100 x"""
    assert K.gradx_emulation_case("gauss", K.MUTATION_SHAPE)[1] <= 1.0
    assert K.gradx_emulation_case("gauss", K.MUTATION_SHAPE, mutate)[1] > 100.0


@pytest.mark.parametrize("mutate", K.GW_MUTATIONS)
def test_gradw_mutations_break_the_bound(mutate):
    """(c) on gauss each misses gw's bound by more than 100 x"""
    assert K.gradw_emulation_case("gauss", K.MUTATION_SHAPE, 3)[1] <= 1.0
    assert K.gradw_emulation_case("gauss", K.MUTATION_SHAPE, 3, mutate)[1] > 100.0


def test_header_declares_and_library_exports_the_entries():
    """(d)"""
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(b2f_ctx \*ctx," % name, hdr), name
        assert name in _lib.SIGNATURES
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(so, name), name
    assert _lib.lib().b2f_version() >= 1015


@pytest.mark.parametrize("shape", K.all_shapes(), ids=_ID)
def test_integers_are_exact(shape):
    """(e) integers without the activation: gw sums products of at most 64, at most 2 x 9 x 33 of them; gx sums multiples of 2^-3 of at most
    4, at most 4 x 192 of them: every partial sum is exact in float32"""
    x, w, _, gy = K.case("integers", shape, False)
    Ci, Co, H, W = shape
    assert K.BATCH * gy.shape[2] * gy.shape[3] * 64 < 2 ** 17 and np.abs(x).max() * np.abs(gy).max() <= 64 and 4 * Co * 4 * 8 < 2 ** 24
    gx, gw, gb = K.backward64(x, w, None, gy, False)
    for P in (1, 3):
        got_w, got_b = K.gradw32(x, K1.masked32(gy, None, False), P)
        assert np.array_equal(got_w.astype(np.float64), gw) and np.array_equal(got_b.astype(np.float64), gb)
    assert np.array_equal(K.gradx_s2_32(gy, w, H, W).astype(np.float64), gx)
