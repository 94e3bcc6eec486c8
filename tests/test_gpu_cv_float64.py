"""GPU: the warp + cost-volume kernels against the float64 restatement of tests/cv_float64.py, at every branch of the launcher.

ops.warp_costvol (NHWC strides) and ops.cv_record (the forward's chunk-planar strides, with flow_b) run under corr_variant = -1; their 162
cost-volume slots must lie within the derived bar (C + 16) * 2^-24 * S of the restatement (cv_float64's docstring derives it), the record's
slots 162..167 must be exactly flow, flow_b and 0, and each of the product variants 0, 1, 3, 5, 7 must give the bits of the automatic run.
The shapes are the smallest that reach each thing (cv_float64.shapes): tiles with all eight neighbours, both sides of the 12-bit
tap-coordinate fields (columns / rows 255|256, 1023|1024, 2047|2048, 4095; maps of 4097 that the unit kernels refuse), and one shape per
branch of the automatic rule, built from the device's CU count -- ops.cv_variant must report the branch each was built for.
ops.costvol runs the generic kernel for windows 3, 5, 7, 11 within the same bar.  Run with -s for the worst ratio and absolute error per
shape and entry (profiles/r16_cv_float64.txt is that printout)."""
import numpy as np
import pytest

from back2future_amd import back2future, ops
from tests import cv_float64 as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PRODUCT_VARIANTS = [0, 1, 3, 5, 7]
SLOT = lambda d, c: c if (d == 0 and c < 80) else (80 + c if c < 80 else 160 + d)      # cv_slot of csrc/b2f_internal.h
SLOTS = [SLOT(d, c) for d in (0, 1) for c in range(81)]
NAMES = [s[0] for s in F.shapes(256)]          # the names do not depend on the CU count, the sizes do


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def table(n_cu):
    return {s[0]: s[1:] for s in F.shapes(n_cu)}


def test_the_shape_list_covers_every_product_variant(table):
    assert sorted(table) == sorted(NAMES)
    assert {F.BRANCH_VARIANT(s[5]) for s in table.values() if s[5] is not None} == {0, 1, 3, 7}      # 5 is never the automatic choice


@pytest.mark.parametrize("name", NAMES)
def test_automatic_rule_takes_the_branch(hard, n_cu, table, name):
    """ops.cv_variant: the launcher's own rule, on both entries' strides; forced variants are reported as forced, and the unit forms report
    variant 3 where warp_costvol_unit_supported refuses the map or the channel count"""
    C, B, h, w, k, branch = table[name]
    layouts = (0, 1) if C % 8 == 0 else (0,)
    with hard.options(corr_variant=-1):
        got = [ops.cv_variant(hard, B, C, h, w, layout) for layout in layouts]
    print("%-16s C %3d %dx%dx%d on %d CUs: variant %s%s" % (name, C, B, h, w, n_cu, got, " (" + branch + ")" if branch else ""))
    assert len(set(got)) == 1 and got[0] in PRODUCT_VARIANTS
    if branch is not None:
        assert got[0] == F.BRANCH_VARIANT(branch), "%s on %d CUs: variant %d, built for '%s'" % (name, n_cu, got[0], branch)
    unit = (C + 7) // 8 * 8 % 16 == 0 and h <= 4096 and w <= 4096
    for variant in PRODUCT_VARIANTS:
        with hard.options(corr_variant=variant):
            for layout in layouts:
                assert ops.cv_variant(hard, B, C, h, w, layout) == (3 if variant in (5, 7) and not unit else variant)


@pytest.mark.parametrize("kind", F.FLOW_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_kernels_meet_the_bar(hard, table, name, kind):
    C, B, h, w, k, branch = table[name]
    seed = C * 1009 + h * 31 + w
    maps = F.make_maps(seed, B, C, h, w)
    flow = F.make_flow(kind, seed + 1, B, h, w, k)
    flow_b = None if flow is None else (flow[:, ::-1] * np.float32(-0.7) + np.float32(0.25)).astype(np.float32)
    val, S = F.warp_costvol64(*maps, flow, k)
    what = "%-16s C %3d %dx%dx%d k %g %-11s" % (name, C, B, h, w, k, kind)
    record = C % 8 == 0                      # C = 20 through ops.warp_costvol only: the padded channels and the Cp / C factor
    with hard.options(corr_variant=-1):
        cv = ops.warp_costvol(hard, *maps, flow, k)
        rec = ops.cv_record(hard, *maps, flow, flow_b, k) if record else None
    for variant in PRODUCT_VARIANTS:
        with hard.options(corr_variant=variant):
            np.testing.assert_array_equal(ops.warp_costvol(hard, *maps, flow, k), cv, err_msg="%s: warp_costvol, variant %d is not the automatic run" % (what, variant))
            if record:
                np.testing.assert_array_equal(ops.cv_record(hard, *maps, flow, flow_b, k), rec, err_msg="%s: cv_record, variant %d is not the automatic run" % (what, variant))
    failures = []
    for entry, got in (("warp_costvol", cv), ("cv_record", rec[:, SLOTS] if record else None)):
        if got is None:
            continue
        try:
            F.check(got, val, S, C, "%s %-12s" % (what, entry))
        except AssertionError as e:          # report both entries before failing
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if record:
        zero = np.zeros_like(rec[:, :2])
        np.testing.assert_array_equal(rec[:, 162:164], flow if flow is not None else zero, err_msg=what + ": slots 162 / 163")
        np.testing.assert_array_equal(rec[:, 164:166], flow_b if flow_b is not None else zero, err_msg=what + ": slots 164 / 165")
        np.testing.assert_array_equal(rec[:, 166:168], zero, err_msg=what + ": slots 166 / 167")


@pytest.mark.parametrize("C,B,h,w", [(6, 2, 11, 13), (8, 1, 1, 2)])
@pytest.mark.parametrize("win", [3, 5, 7, 11])
def test_generic_windows(hard, win, C, B, h, w):
    """ops.costvol on the generic kernel (the second shape: a map smaller than the window)"""
    r = np.random.default_rng(win * 100 + C)
    ref = r.standard_normal((B, C, h, w), dtype=np.float32)
    frm = r.standard_normal((B, C, h, w), dtype=np.float32)
    for fwd in (True, False):
        val, S = F.costvol64(ref, frm, win, fwd)
        F.check(ops.costvol(hard, ref, frm, win, fwd), val, S, C, "costvol win %2d %s C %d %dx%dx%d" % (win, "fwd" if fwd else "bwd", C, B, h, w))
