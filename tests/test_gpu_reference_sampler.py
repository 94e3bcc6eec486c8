"""GPU: the bilinear sampler pinned to the reference's own kernels -- extras/stnbhwd/BilinearSamplerBHWD.cu compiled unmodified by
oracle/reference.py into oracle/_ref/ -- and to the float64 restatement with counted bounds of tests/sampler_float64.py, on that
helper's seven shapes and four grids (B = 2).

(a) the compiled reference, the contraction-off build and the default (contracting) one, within n 2^-24 S of float64: forward n = 5, grid
    gradient n = ceil(C / 32) + 9 in full and only-grid form, image gradient n = K + 1 per element (0 where S = 0);
(b) the CPU oracle against the contraction-off reference bit for bit: warp_bhwd, the grid gradient of warp_bhwd_backward in both forms,
    warping_unit for k = -20, 20, 2.5.  Derived, not measured: with contraction off both sides run one fixed sequence of float32
    operations -- the blend left to right, per-lane sums with stride 32, the 16 / 8 / 4 / 2 / 1 tree.  The oracle's image gradient adds in
    another order than the atomics: held to float64 within its bound and to the reference's within the two bounds added;
(c) the library against the contraction-off reference: ops.warp_bhwd (warp_nhwc_kernel) and the grid gradient of
    ops.warp_bhwd_backward (warp_bhwd_backward_kernel) in both forms bit for bit -- the kernels' expressions are in the reference's order
    and libb2f.so is built without contraction --, the image gradient (atomics on both sides) against float64 within its bound;
(d) the contracting build is held to the float64 bounds only; its distance from the contraction-off build in units of 2^-24 S is printed
    (-s), profiles/r28_reference_sampler.txt is that printout.
Skipped only where oracle/_ref/libref_sampler.so does not exist."""
import functools
import os

import numpy as np
import pytest

from back2future_amd import back2future, ops
from oracle import oracle as O
from oracle import reference as REF
from tests import sampler_float64 as SF

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(REF.lib_path()), reason="oracle/_ref/libref_sampler.so does not exist")]

f32 = np.float32
DIST = {}          # (quantity, field) -> the contracting build's largest distance from the contraction-off build, in 2^-24 S
WORST = {}         # (who, quantity) -> [worst err / (2^-24 S) (image gradient: / the bound), bound]


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n%-28s %-16s %12s %8s" % ("who", "quantity", "worst/(uS)", "bound n"))
    for (who, q), (r, n) in sorted(WORST.items()):
        print("%-28s %-16s %12.3f %8s" % (who, q, r, n))
    print("\ncontracting build - contraction-off build, largest |difference| / (2^-24 S) per output")
    print("%-16s" % "quantity" + "".join("%10s" % f for f in SF.FIELDS))
    for q in ("forward", "grid gradient", "image gradient"):
        print("%-16s" % q + "".join("%10.3f" % DIST.get((q, f), float("nan")) for f in SF.FIELDS))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _differ(a, b):
    """how many elements differ in their bits (-1: the shapes do)"""
    return -1 if a.shape != b.shape else int((_bits(a) != _bits(b)).sum())


@functools.lru_cache(maxsize=None)
def compiled(case, field, fma=False):
    """the compiled reference on one case and field, run once and shared (read-only): forward, image gradient, grid gradient, only-grid"""
    R = SF.reference(case, field)
    gi, gg = REF.backward(R["img"], R["grid"], R["grad_out"], fma=fma)
    none, gg_only = REF.backward(R["img"], R["grid"], R["grad_out"], only_grid=True, fma=fma)
    assert none is None
    out = dict(fwd=REF.forward(R["img"], R["grid"], fma=fma), gi=gi, gg=gg, gg_only=gg_only)
    for a in out.values():
        a.setflags(write=False)
    return out


def _bound(fails, who, quantity, what, got, val, S, n, per_element=None):
    """|got - val| <= n 2^-24 S (per_element: n varies, S already carries it and the figure is in units of the bound)"""
    r = SF.measure(got, val, S)
    t = WORST.setdefault((who, quantity), [0.0, "K + 1" if per_element else n])
    t[0] = max(t[0], r)
    if not per_element:
        t[1] = max(t[1], n)          # the table shows the largest n of the shapes
    print("%-46s %-26s %-16s err / (u S) = %8.3f (n = %s)" % (what, who, quantity, r, "K + 1" if per_element else n))
    if not r <= (1 if per_element else n):
        fails.append("%s %s %s: %.3f exceeds %s" % (what, who, quantity, r, "the bound (K + 1) u S" if per_element else "n = %d" % n))


def _float64_bounds(fails, who, what, case, R, fwd, gg, gg_only, gi):
    if fwd is not None:
        _bound(fails, who, "forward", what, fwd, *R["fwd"], SF.N_FORWARD)
    for q, g in (("grid gradient", gg), ("only-grid", gg_only)):
        if g is not None:
            _bound(fails, who, q, what, g, *R["gg"], SF.n_grid(case[0]))
    if gi is not None:
        val, S, K = R["gi"]
        _bound(fails, who, "image gradient", what, gi, val, S * SF.n_image(K), None, per_element=True)


# ---- (a), (d): the compiled reference against float64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SF.CASES, ids=SF.case_id)
def test_compiled_reference_within_float64_bounds(case):
    fails = []
    for field in SF.FIELDS:
        R = SF.reference(case, field)
        what = "%s %s" % (SF.case_id(case), field)
        for fma in (False, True):
            got = compiled(case, field, fma)
            _float64_bounds(fails, "reference, contracting" if fma else "reference, contraction off", what, case, R, got["fwd"], got["gg"], got["gg_only"],
                            got["gi"])
            if _differ(got["gg"], got["gg_only"]):          # one template, one sequence of operations
                fails.append("%s fma %d: the only-grid form differs from the full one in %d components" % (what, fma, _differ(got["gg"], got["gg_only"])))
        off, on = compiled(case, field, False), compiled(case, field, True)
        for q, key, S in (("forward", "fwd", R["fwd"][1]), ("grid gradient", "gg", R["gg"][1]), ("image gradient", "gi", R["gi"][1])):
            DIST[(q, field)] = max(DIST.get((q, field), 0.0), SF.distance(on[key], off[key], S))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


# ---- (b): the oracle against the contraction-off reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SF.CASES, ids=SF.case_id)
def test_oracle_is_the_compiled_reference(case):
    fails = []
    for field in SF.FIELDS:
        R = SF.reference(case, field)
        ref = compiled(case, field)
        what = "%s %s" % (SF.case_id(case), field)
        n = _differ(O.warp_bhwd(R["img"], R["grid"]), ref["fwd"])
        if n:
            fails.append("%s: oracle.warp_bhwd differs from the reference in %d outputs" % (what, n))
        gi, gg = O.warp_bhwd_backward(R["img"], R["grid"], R["grad_out"])
        none, gg_only = O.warp_bhwd_backward(R["img"], R["grid"], R["grad_out"], only_grid=True)
        assert none is None
        for form, g, r in (("full", gg, ref["gg"]), ("only-grid", gg_only, ref["gg_only"])):
            n = _differ(g, r)
            if n:
                fails.append("%s: the oracle's grid gradient (%s) differs from the reference's in %d components" % (what, form, n))
        _float64_bounds(fails, "oracle", what, case, R, None, None, None, gi)
        val, S, K = R["gi"]
        if not SF.measure(gi, ref["gi"].astype(np.float64), 2.0 * S * SF.n_image(K)) <= 1:
            fails.append("%s: the oracle's image gradient is further from the reference's than the two bounds added" % what)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("case", [c for c in SF.CASES if c[1:3] == c[3:5]], ids=SF.case_id)
def test_oracle_warping_unit_is_the_compiled_reference(case):
    """warpingUnit (models/pwc.lua:67-73) behind MulConstant(k): the transposes and the float32 product around the compiled sampler"""
    fails = []
    for field in SF.FIELDS:
        for k in SF.UNIT_K:
            I, F = SF.unit_inputs(case, field, k)
            n = _differ(O.warping_unit(I, F, k), REF.warping_unit(I, F, k))
            if n:
                fails.append("%s %s k %g: oracle.warping_unit differs from the reference in %d outputs" % (SF.case_id(case), field, k, n))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


# ---- (c): the library against the contraction-off reference -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SF.CASES, ids=SF.case_id)
def test_library_is_the_compiled_reference(hard, case):
    fails = []
    for field in SF.FIELDS:
        R = SF.reference(case, field)
        ref = compiled(case, field)
        what = "%s %s" % (SF.case_id(case), field)
        fwd = ops.warp_bhwd(hard, R["img"], R["grid"])
        n = _differ(fwd, ref["fwd"])
        if n:
            fails.append("%s: ops.warp_bhwd differs from the reference in %d outputs" % (what, n))
        gi, gg = ops.warp_bhwd_backward(hard, R["img"], R["grid"], R["grad_out"])
        none, gg_only = ops.warp_bhwd_backward(hard, R["img"], R["grid"], R["grad_out"], only_grid=True)
        assert none is None
        for form, g, r in (("full", gg, ref["gg"]), ("only-grid", gg_only, ref["gg_only"])):
            n = _differ(g, r)
            if n:
                fails.append("%s: the library's grid gradient (%s) differs from the reference's in %d components" % (what, form, n))
        _float64_bounds(fails, "library", what, case, R, fwd, gg, gg_only, gi)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)
