"""No GPU: the yardstick of the conv layer's backward pass (tests/conv_backward_float64.py) against torch.autograd, the float32 emulation of
the gradWeight split against its bound and the recorded ratios, the mutations the bound must catch, and the C ABI's two new entries."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from back2future_amd import _lib
from tests import conv_backward_float64 as K
from tests import conv_float64 as F

ROOT = F.ROOT
ENTRIES = ("b2f_op_conv3x3_backward", "b2f_op_conv3x3_backward_plan")


def _autograd(x, w, b, gy, leaky):
    """(y, gx, gw, gb) of conv2d + leaky_relu(0.2) in float64"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    xt, wt, bt = t(x).requires_grad_(), t(w).requires_grad_(), t(b).requires_grad_()
    y = torch.nn.functional.conv2d(xt, wt, bt, padding=1)
    if leaky:
        y = torch.nn.functional.leaky_relu(y, 0.2)
    y.backward(t(gy))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("leaky", [False, True])
def test_backward64_is_autograd(family, leaky):
    """(a) to 1e-12 of the largest magnitude.  The saved output here is autograd's own float64 y, so the mask is the same wherever y != 0;
    the elements forced to y == 0 are compared after forcing the slope by hand: the gradient there is 0.2 gy whatever torch chooses at 0."""
    Ci, Co, H, W = 40, 36, 17, 33
    x, w, b = F.make_case(family, K.SEED, K.BATCH, Ci, Co, H, W)
    gy = F.make_case(family, K.SEED + 1, K.BATCH, Co, Ci, H, W)[0].astype(np.float64)
    y, gx, gw, gb = _autograd(x, w, b, gy, leaky)
    for got, want in zip(K.backward64(x, w, y, gy, leaky), (gx, gw, gb)):
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    if not leaky:
        return
    zero = np.random.default_rng(5).random(y.shape) < 0.03
    y0 = np.where(zero, 0.0, y)
    # by hand: where y was positive and is now 0, the slope replaces the 1
    g_forced = np.where(y0 > 0, gy, 0.2 * gy)
    assert (g_forced != np.where(y > 0, gy, 0.2 * gy)).any()
    want = _autograd_from_g(x, w, g_forced)
    for got, ref in zip(K.backward64(x, w, y0, gy, True), want):
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)


def _autograd_from_g(x, w, g):
    """(gx, gw, gb) of the convolution alone for the output gradient g, by autograd in float64"""
    return _autograd(x, w, np.zeros(w.shape[0]), g, False)[1:]


@pytest.mark.parametrize("shape", K.all_shapes(), ids=lambda s: "%dto%d-%dx%d" % s)
def test_emulation_stays_within_the_bound(shape):
    """(b) gradw32 within bound_gw, gb within the same bound, every family, P in {1, 3}"""
    for family in F.FAMILIES:
        for P in (1, 3):
            rw, rw_bound, rb, rb_bound = K.emulation_case(family, shape, P)
            assert rw_bound <= 1.0 and rb_bound <= 1.0, (family, P, rw, rw_bound, rb, rb_bound)


def test_recorded_ratios_are_fresh():
    """(b) tests/golden/conv_backward_ratios.json is what `python -m tests.conv_backward_float64` writes now"""
    fresh, rec = K.compute_ratios(), K.recorded_ratios()
    assert set(fresh) == set(rec) == set(F.FAMILIES)
    for fam in F.FAMILIES:          # the tolerance of tests/test_conv_float64_cpu.py: the float64 sums are BLAS's, whose order is the machine's
        assert abs(fresh[fam] - rec[fam]) <= 1e-3 * rec[fam] + 1e-6, (fam, fresh[fam], rec[fam])
    assert json.load(open(K.RATIOS_PATH)) == rec


@pytest.mark.parametrize("mutate", K.MUTATIONS)
def test_mutations_break_the_bound(mutate):
    """(c) each of the five, on gauss, misses its bound by more than 100 x"""
    shape = K.MUTATION_SHAPE
    if mutate in ("no-rotation", "no-transpose"):
        assert K.gradx_mutation_case("gauss", shape, None) <= 1.0
        assert K.gradx_mutation_case("gauss", shape, mutate) > 100.0
        return
    assert K.emulation_case("gauss", shape, 3)[1] <= 1.0
    assert K.emulation_case("gauss", shape, 3, mutate)[1] > 100.0
    if mutate == "mask-from-gy":
        assert K.gradx_mutation_case("gauss", shape, mutate) > 100.0


def test_header_declares_and_library_exports_the_entries():
    """(d)"""
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(b2f_ctx \*ctx," % name, hdr), name
        assert name in _lib.SIGNATURES
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(so, name), name
    assert _lib.lib().b2f_version() >= 1014


@pytest.mark.parametrize("shape", K.all_shapes(), ids=lambda s: "%dto%d-%dx%d" % s)
def test_integers_are_exact(shape):
    """(e) integers without the activation: products of at most 64, at most 1 274 of them (2 x 13 x 49): every partial sum is an integer
    below 2^17"""
    x, w, _, gy = K.case("integers", shape, False)
    assert K.BATCH * shape[2] * shape[3] * 64 < 2 ** 17 and np.abs(x).max() * np.abs(gy).max() <= 64
    _, gw, gb = K.backward64(x, w, None, gy, False)
    for P in (1, 3):
        got_w, got_b = K.gradw32(x, K.masked32(gy, None, False), P)
        assert np.array_equal(got_w.astype(np.float64), gw) and np.array_equal(got_b.astype(np.float64), gb)
