"""GPU: the generic executor (graph_run, csrc/b2f_graph.hip) under guard bands and a NaN fill, on weights that displace.

tests/test_gpu_guards.py holds the shipped graph's plans to the contract "a kernel may read outside its tensors only if the value cannot
reach a result, and may write nowhere outside them"; this module holds the executor of every other option set of createModelMulti to it.
With arena_guard = 4096 and arena_fill = 1 the executor's own layout of the arena -- some twenty buffers per level, each named by role
and level -- has 4096 floats of 0x7fc0a5a5 in front of the first buffer and behind every buffer, the arena is refilled whenever a pass lays
it out differently, and the tensors of b2f_forward's output table are guarded buffers that start as that word.  One guarded and one
plain context per (case, kind) of tests/test_graph_options_cpu.py's CASES run the same calls: their tables are bit-identical,
b2f_arena_check is clean after every call, and the plain context's tables are those of a context that has seen nothing else.

The weights are tests/displaced.py's for the graph (image warps of about 3 pixels through the clamp at every level, occlusion planes
with values on both sides of the threshold; with occ_input the levels calibrated coarsest first), whose conditions are asserted on the
oracle's table before anything is compared; tests/test_graph_displaced_cpu.py shows on the CPU that the oracle stays within 1e-3 of the
float64 witness on them and that a wrong graph constant moves the table by far more.  Here the GPU's table is held to the same 1e-3
(BASELINE.json) against the float64 witness and against the oracle.  Run with -s for |gpu - f64| beside |oracle - f64|
(profiles/r22_graph_displaced.txt)."""
import numpy as np
import pytest

from back2future_amd import _lib, back2future, weights as W
from tests import displaced as D
from tests.test_gpu_displaced import KERNEL_SETTINGS
from tests.test_gpu_guards import GUARD, _assert_bit_equal, _assert_clean
from tests.test_graph_displaced_cpu import BAR, CASES, KINDS, SIZES, TINY, graph_case, tensor_kinds, worst_by_kind

pytestmark = pytest.mark.gpu

ORDER = [SIZES[0], TINY, SIZES[1], SIZES[0]]        # a smaller call after a larger one on the grown arena, and back
WIDE_SETTINGS = ["f4x4", "f6x6", "wino1d-2", "bf16-wide", "bf16_conv-0"]
WIDE_CASES = ["occ_input+rescale", "sum_cvs"]       # decoder inputs of 86 / 84 and 84 / 59 channels: counts the shipped graph never has


def _model(name, which, guarded=False):
    o = W.graph_opts(**CASES[name])
    m = back2future.Model("random:%s:%d:2.0" % (which, 5), graph=W.opts_string(o))
    if guarded:
        m.set_option("arena_guard", GUARD)
        m.set_option("arena_fill", 1)
    return m


_pairs = {}


def _pair(name, which):
    """(guarded context, plain context) of a case and kind, on the displaced weights of the largest size"""
    if (name, which) not in _pairs:
        flat = graph_case(name, which, *SIZES[0])[2]
        g, p = _model(name, which, True), _model(name, which)
        g.set_weights(flat)
        p.set_weights(flat)
        _pairs[(name, which)] = (g, p)
    g, p = _pairs[(name, which)]
    assert g.get_option("arena_guard") == GUARD and g.get_option("arena_fill") == 1
    assert p.get_option("arena_guard") == 0 and p.get_option("arena_fill") == 0
    return g, p


def _close_pair(key):
    for m in _pairs.pop(key, ()):
        m.close()


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for key in list(_pairs):
        _close_pair(key)


def _what(name, which, x, step=None):
    return "%s %s %dx%dx%d%s" % (name, which, x.shape[0], x.shape[2], x.shape[3], "" if step is None else " (call %d)" % (step + 1))


# ---- the sizes in their order: guarded against plain, warm against fresh, GPU against float64 ----

@pytest.mark.parametrize("which", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_sizes_in_order(name, which):
    """b2f_forward at 2 x 4m x 6m, 1 x m x m, 1 x 3m x 5m and 2 x 4m x 6m again (m = 2^(levels - 1): coarsest maps of 4 x 6, one pixel and
    3 x 5), each on the weights calibrated for its size (one pixel: those of the largest).  After every call: the guarded context's table
    is the plain one's bit for bit and no guard word has changed; the plain context's table is that of a fresh context which has only
    seen this size (nothing stale in a grown workspace reaches a result); and at the two larger sizes every tensor is within 1e-3 of the
    float64 witness and of the oracle, whose table meets displaced.conditions."""
    past = which == "soft"
    g, p = _pair(name, which)
    try:
        for step, size in enumerate(ORDER):
            o, x, flat, table, ref = graph_case(name, which, *size)
            what = _what(name, which, x, step)
            if size != TINY:
                D.assert_conditions(table, past, o, D.CASE_BOUNDS.get(name))
            for m in (g, p):
                m.set_weights(flat)
            got = g.forward(x)
            _assert_clean(g, what)
            exp = p.forward(x)
            assert len(got) == len(exp) == len(table)
            assert all(np.isfinite(a).all() for a in exp), what
            _assert_bit_equal(got, exp, what)
            fresh = _model(name, which)
            try:
                fresh.set_weights(flat)
                _assert_bit_equal(exp, fresh.forward(x), what + ": warm context against a fresh one")
            finally:
                fresh.close()
            if size == TINY or step == len(ORDER) - 1:
                continue
            e64, eor, o64 = worst_by_kind(exp, ref, past), worst_by_kind(exp, table, past), worst_by_kind(table, ref, past)
            for k in tensor_kinds(past):
                print("graph %-28s %s %dx%dx%d %-4s |gpu - f64| %.3g  |oracle - f64| %.3g  ratio %.2f  |gpu - oracle| %.3g"
                      % (name, which, x.shape[0], x.shape[2], x.shape[3], k, e64[k], o64[k], e64[k] / max(o64[k], 1e-30), eor[k]))
            assert max(e64.values()) <= BAR and max(eor.values()) <= BAR, (what, e64, eor)
    finally:
        _close_pair((name, which))


# ---- every kernel a user can select, on decoder widths the shipped graph never has ----

def _first_layer_rows(rows, o, past, h, w):
    """{row: count} of the first decoder layers of the finest level (profile_layers: conv<tag>_<padded inputs>to128_<h>x<w>) and the
    number of decoders that must be among them"""
    l = D.graph_levels(o)[0]
    widths = {(n + 7) // 8 * 8 for n in (W.occ_in_ch(l, o), W.flow_in_ch(l, o))}
    return {n: c for n, c in rows.items() if any(n.endswith("_%dto128_%dx%d" % (ci, h, w)) for ci in widths)}, 3 if past else 2


@pytest.mark.parametrize("setting", WIDE_SETTINGS)
@pytest.mark.parametrize("which", KINDS)
@pytest.mark.parametrize("name", WIDE_CASES)
def test_every_selectable_kernel(name, which, setting):
    """The wide-layer settings of tests/test_gpu_displaced.py at 2 x 4m x 6m: F(4x4), F(6x6), the 1-D Winograd kernel, the bf16 pipe and
    the fp32 direct kernel on decoder inputs of 88 and 64 padded channels behind put_channels' zero pad.  Guarded and plain agree bit
    for bit, the guards are clean, the 1e-3 bars hold, and the profile rows name the kernel the finest level's first decoder layers ran on."""
    past = which == "soft"
    o, x, flat, table, ref = graph_case(name, which, *SIZES[0])
    D.assert_conditions(table, past, o, D.CASE_BOUNDS.get(name))
    g, p = _pair(name, which)
    opts, tag = KERNEL_SETTINGS[setting]
    opts = dict({"adaptive_kernels": 0}, **opts)
    what = _what(name, which, x) + " " + setting
    with g.options(**opts), p.options(**opts):
        got = g.forward(x)
        _assert_clean(g, what)
        with p.options(profile=1, profile_layers=1):
            p.profile_reset()
            exp = p.forward(x)
            rows = {n: cnt for n, (ms, cnt) in p.profile_read().items() if cnt > 0}
    _assert_bit_equal(got, exp, what)
    e64, eor = worst_by_kind(exp, ref, past), worst_by_kind(exp, table, past)
    print("graph %-20s %s %-12s %s" % (name, which, setting, "  ".join("%s %.3g / %.3g" % (k, e64[k], eor[k]) for k in e64)))
    assert all(np.isfinite(a).all() for a in exp), what
    assert max(e64.values()) <= BAR and max(eor.values()) <= BAR, (what, e64, eor)
    s = 1 << (D.graph_levels(o)[0] - 1)
    first, n = _first_layer_rows(rows, o, past, x.shape[2] // s, x.shape[3] // s)
    print("graph %-20s %s %-12s first decoder layers of the finest level: %s" % (name, which, setting, first))
    assert sum(first.values()) == n, (first, sorted(rows))
    if tag:
        assert all(r.startswith("conv%s_" % tag) for r in first), first


# ---- the other entries over the same executor ----

def test_compute_flow_and_forward_loss():
    """createModelMulti(nil), Soft: computeFlow (the context-owned output table of forward_device) and forwardLoss (forward_table_run
    into the loss workspace) lay the arena out through the same executor: guarded and plain agree bit for bit, the guards are clean"""
    name, which = "createModelMulti(nil)", "soft"
    o, x, flat, table, ref = graph_case(name, which, *SIZES[0])
    g, p = _pair(name, which)
    rng = np.random.default_rng(21)
    ims = [rng.random((3, 72, 100), dtype=np.float32) for _ in range(3)]
    got = g.computeFlow(*ims)
    _assert_clean(g, "computeFlow")
    _assert_bit_equal(got, p.computeFlow(*ims), "computeFlow")
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0.1
    rec_g, tab_g = g.forwardLoss(x, want_table=True)
    _assert_clean(g, "forwardLoss")
    rec_p, tab_p = p.forwardLoss(x, want_table=True)
    _assert_bit_equal([rec_g] + list(tab_g), [rec_p] + list(tab_p), "forwardLoss")
    _assert_bit_equal(tab_p, p.forward(x), "forwardLoss's table against forward's")
    _assert_bit_equal(got, g.computeFlow(*ims), "computeFlow after another shape")
    _assert_clean(g, "computeFlow after another shape")


# ---- the detectors detect on the executor's layout ----

def test_selftest_names_the_generic_buffers():
    """One guard word overwritten by a copy from the host (no kernel stores out of range): b2f_arena_check reports that word, under the
    name the executor gave the buffer -- its role and level"""
    name, which = "occ_input+rescale", "soft"
    o, x, flat, table, ref = graph_case(name, which, *SIZES[1])
    m = _model(name, which, True)
    try:
        m.set_weights(flat)
        assert m.arena_check() == 0
        with pytest.raises(_lib.B2FError, match="no guarded plan"):
            m.guard_selftest(0)
        m.forward(x)
        assert m.arena_check(detail=True)[:3] == (0, -1, 0)
        m.guard_selftest(0)                                  # the executor's buffers start img, ds[2], ds[3], tmp, cs[2], ...
        n, buf, off, msg = m.arena_check(detail=True)
        assert (n, buf, off) == (1, 1, 3) and "after buffer 'ds[2]'" in msg and "0x3f800000" in msg, (n, buf, off, msg)
        m.guard_selftest(1)
        n, buf, off, msg = m.arena_check(detail=True)
        assert (n, buf, off) == (2, 0, -2) and "before buffer 'img'" in msg, (n, buf, off, msg)
        m.forward(x)                                         # the same layout: no refill, the two words stay
        assert m.arena_check() == 2
        m.forward(graph_case(name, which, *SIZES[0])[1])     # another shape: filled afresh
        assert m.arena_check() == 0
    finally:
        m.close()
