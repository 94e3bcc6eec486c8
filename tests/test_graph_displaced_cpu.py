"""CPU: the displaced weights of tests/displaced.py on every graph shape of tests/test_graph_options_cpu.py's CASES -- what
tests/test_gpu_graph_guards.py holds the generic executor to, shown to hold for the reference alone first.

For every case x {hard, soft} x size: displaced.conditions on the oracle's table (whole-pixel image warps through the clamp at every
level, occlusion planes with values on both sides of the threshold), and every tensor of the oracle's table within the 1e-3 of
BASELINE.json of the float64 witness tests/torch_ref.py::pwc_forward -- the oracle itself stays inside the bar the GPU is held to, with
room (the figures: displaced.py's table; run with -s).  Then the point of the weights: one wrong graph constant moves the table by more
than ten times that bar."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from back2future_amd import weights as W
from oracle import oracle as O
from tests import displaced as D
from tests import torch_ref as R
from tests.test_graph_options_cpu import CASES

torch.set_num_threads(4)

SEED, DISP, SPREAD = 5, 3.0, 1.0
BAR = 1e-3                                  # BASELINE.json: max-abs on flow / occlusion probabilities / the output table
KINDS = ["hard", "soft"]
SIZES = [(2, 4, 6), (1, 3, 5)]              # (B, H / m, W / m), m = 2^(levels - 1): the coarsest map is 4 x 6 / 3 x 5
TINY = (1, 1, 1)                            # a coarsest map of one pixel: no quartiles to calibrate on


def tensor_kinds(past):
    return ["ufs", "ubfs", "occs", "iw1", "iw3"] if past else ["ufs", "occs", "iw1", "iw3"]


def case_input(o, past, B, a, b):
    m = 1 << (o["levels"] - 1)
    H, Wd = a * m, b * m
    return np.random.default_rng(H + Wd + past).standard_normal((B, 9, H, Wd)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def graph_case(name, which, B, a, b):
    """(o, x, weights, the oracle's table, the float64 witness's table) of one case, kind and size; computed once per session and never
    written to.  At TINY the weights are those of the largest size (as tests/test_gpu_guards.py::_case does for its 64 x 64)."""
    o = W.graph_opts(**CASES[name])
    past = which == "soft"
    x = case_input(o, past, B, a, b)
    flat = graph_case(name, which, *SIZES[0])[2] if (B, a, b) == TINY else D.displaced_weights(SEED, past, x, DISP, SPREAD, o=o)
    table = O.pwc_forward(x, flat, past, D.oracle_opts(o, past))
    ref, _ = R.pwc_forward(x, W.views(flat, past, o), past, o=o)
    for t in table + ref:
        t.setflags(write=False)
    return o, x, flat, table, ref


def worst_by_kind(got, exp, past):
    """{tensor kind: max |got - exp| over the levels}, in float64"""
    kinds = tensor_kinds(past)
    worst = dict.fromkeys(kinds, 0.0)
    assert len(got) == len(exp) and len(got) % len(kinds) == 0
    for i, (a, b) in enumerate(zip(got, exp)):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        k = kinds[i % len(kinds)]
        worst[k] = max(worst[k], float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))
    return worst


def _assert_within_bar(name, which, size):
    o, x, flat, table, ref = graph_case(name, which, *size)
    past = which == "soft"
    assert len(table) == (o["levels"] - o["skip"]) * (5 if past else 4)
    assert all(np.isfinite(t).all() for t in table) and all(np.isfinite(t).all() for t in ref)
    worst = worst_by_kind(table, ref, past)
    print("oracle - float64 %-28s %s %dx%dx%d: %s" % (name, which, x.shape[0], x.shape[2], x.shape[3],
                                                       "  ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= BAR, worst


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dmx%dm" % s)
@pytest.mark.parametrize("which", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_conditions_and_float64(name, which, size):
    o, x, flat, table, ref = graph_case(name, which, *size)
    for line in D.assert_conditions(table, which == "soft", o, D.CASE_BOUNDS.get(name)):
        print("conditions %s %s %s: %s" % (name, which, x.shape, line))
    _assert_within_bar(name, which, size)


@pytest.mark.parametrize("which", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_pixel_coarsest_map(name, which):
    _assert_within_bar(name, which, TINY)


# ---- one wrong graph constant ----

def _zero_occ_input(flat, past, o):
    """the occlusion decoders' first layers blind to the last two input channels, the upsampled occlusion map of the level above"""
    flat = flat.copy()
    v = W.views(flat, past, o)
    for l in range(D.graph_levels(o)[0], o["levels"]):
        v["l%d.occ.conv1.w" % l][:, -2:] = 0
    return flat


def _mutations(o, past):
    """(name, options, weight edit) of every mutation that applies to the graph: an option is flipped only where the flip keeps the
    parameter count, so that the same weights run"""
    n = W.param_count(past, o)
    out = [("flownet_factor / 2", dict(o, flownet_factor=o["flownet_factor"] / 2), None)]
    for key in ("rescale_flow", "occ_input", "sum_cvs"):
        m = dict(o, **{key: 1 - o[key]})
        if key == "sum_cvs" and o["two_frame"]:
            continue                        # pwc.lua:279-283: a two_frame graph has one cost volume and does not read the option
        if W.param_count(past, m) == n:
            out.append((key + " flipped", m, None))
    if o["occ_input"]:
        out.append(("occ_input channels unread", o, _zero_occ_input))
    return out


def _todays_weights(o, past):
    """what tests/test_gpu_graph_options.py runs on"""
    return D.set_flow_bias(W.random_init(11, past, 2.0, o), past, (0.35, -0.25), o)


@pytest.mark.parametrize("which", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_wrong_graph_constant_moves_the_table(name, which):
    """The errors the generic executor can make in its constants -- k / k2 of the warps from flownet_factor and rescale_flow, the x 2 of
    rescale_flow's upsampling, the channel offset of the occlusion input -- as the same error in the oracle: each moves at least one
    tensor of the displaced table by more than 10 x the bar.  Beside it, the same mutation on the weights of
    tests/test_gpu_graph_options.py.

    occ_input and sum_cvs change the decoders' input widths, so their flips never keep the parameter count and do not run (sum_cvs
    keeps it only under two_frame, which does not read it); what occ_input adds is covered by "occ_input channels unread": the
    occlusion decoders' first layers with zero weights on the two channels of the upsampled occlusion map, as if a wrong offset had
    put the map where the zero pad is.

    Measured at 2 x 4m x 6m over the 22 (case, kind) pairs, displaced / today's weights, largest difference over the table:
    flownet_factor / 2 moves it by 3.7 .. 5.7 / 3.8 .. 5.8 and rescale_flow flipped by 3.1 .. 10 / 3.4 .. 11 -- both through the
    warped images, which on a standard-normal input move by the image's own range under any flow error, so today's weights see these
    two as well; occ_input channels unread moves the occlusion maps (nothing else reads them) by 0.32 .. 0.61 / 0.030 .. 0.059: under
    today's weights the decoders all but ignore the map of the level above, and a wrong offset there would have stayed within 60 x the
    bar where it now stands at 300 .. 600 x.  Every mutation reaches the factor 10 at this size on the displaced weights."""
    o, x, flat, table, _ = graph_case(name, which, *SIZES[0])
    past = which == "soft"
    old = _todays_weights(o, past)
    old_table = O.pwc_forward(x, old, past, D.oracle_opts(o, past))
    missed = []
    for what, m, edit in _mutations(o, past):
        figures = []
        for w, t in ((flat, table), (old, old_table)):
            got = O.pwc_forward(x, edit(w, past, m) if edit else w, past, D.oracle_opts(m, past))
            figures.append(worst_by_kind(got, t, past))
        print("mutation %-28s %s %-26s moves, displaced / today's weights: %s" % (name, which, what, "  ".join(
            "%s %.3g / %.3g" % (k, figures[0][k], figures[1][k]) for k in figures[0])))
        if not max(figures[0].values()) > 10 * BAR:
            missed.append((what, figures[0]))
    assert not missed, missed


# ---- the shipped graph's weights have not moved ----

# sha256 of displaced_weights(5, past, x, 3.0, 1.0) as the commit before the option argument computed it, on the inputs of
# tests/test_gpu_displaced.py::_table_case
SHIPPED_DIGESTS = {
    ("hard", 2, 128, 192): "82effcde4c996650cfe3b3a4d9acd9baf89fcf5f2472e9337a181fb44256563c",
    ("hard", 1, 192, 320): "f097d7eef6b3e54fdee818f0e1ae87a54f67022d9b01cbfd5cb3485f6dd20f97",
    ("soft", 2, 128, 192): "428a9980b4ad4233fc245cbd43aea3e74cf59cd4a83df84272abeee824545da1",
    ("soft", 1, 192, 320): "42950e4fed348c6f34f8436ad7ab12726867448e2444d8211c05d868f933b02b",
}


@pytest.mark.parametrize("which,B,H,Wd", sorted(SHIPPED_DIGESTS))
def test_shipped_displaced_weights_are_unchanged(which, B, H, Wd):
    past = which == "soft"
    x = np.random.default_rng(H + Wd + past).standard_normal((B, 9, H, Wd)).astype(np.float32)
    for flat in (D.displaced_weights(SEED, past, x, DISP, SPREAD), D.displaced_weights(SEED, past, x, DISP, SPREAD, o=W.graph_opts())):
        assert hashlib.sha256(flat.tobytes()).hexdigest() == SHIPPED_DIGESTS[(which, B, H, Wd)]
    assert D.table_index(past, 5, "occs") == (12 if past else 9) and D.level_bias(3.0)(4) == (3.0 * 2.0 / 20.0, 3.0 * -0.7 * 2.0 / 20.0)
