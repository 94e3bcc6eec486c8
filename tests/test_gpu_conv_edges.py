"""GPU: every conv kernel swept over the edges of its tile and of its block, against the float64 restatement of tests/conv_float64.py.

tests/test_gpu_conv_float64.py holds the kernels to the derived bound on five shapes per class; the code a rewrite of a kernel touches is
the ragged last tile and the ragged last block of a map.  conv_float64.GEOMETRY names each kernel's tile (th, tw) and block footprint
(bh, bw); edge_shapes turns a row into output sizes that hold every residue of the tile, one under / on / one over the footprint, a size
over two footprints and every multiple of 8 below it, in both dimensions (stride 2: from an odd and from an even input).  One case = one
(kernel id, channel configuration of conv_float64.EDGE_CHANNELS: one per block form of the kernel) over the id's whole sweep and the
families gauss, dc, integers, batch 2 with different images, under the options CONFIGS uses to force the kernel.  Per call:

  * the profile row names the kernel the case is meant for (a last n-block of <= 32 outputs as _channel_groups states it);
  * |got - conv64| <= n u S elementwise, S the yardstick of the algorithm that computed the channel (conv_float64.bound: the derived bar,
    no tolerance of this file's own); where every product is zero, exactly the bias through the LeakyReLU;
  * integers: bit for bit where CONFIGS flags the kernel exact;
  * a guard of the op entry's staging scope that was written, or a buffer left unwritten, raises in the entry and fails the case;
  * under the options of CONFIGS' other launcher branches `gauss` gives the same bits.

ops.conv_head16 and ops.conv_first (with and without ColorNormalize) run their own sweeps.  The table printed at the end (-s;
profiles/r31_conv_edges.txt is that printout) gives, per kernel and family, the worst err / (u S) on the border ring -- the pixels whose tile
is ragged or touches the map's edge -- and in the interior."""
import time

import numpy as np
import pytest

from back2future_amd import ops
from back2future_amd._lib import B2FError
from tests import conv_float64 as F
from tests.test_gpu_conv_float64 import CONFIGS, EXPERIMENTS, _channel_groups, _ran
from tests.test_gpu_conv_float64 import hard          # noqa: F401  (the module-scoped model fixture)

pytestmark = pytest.mark.gpu

CASES = [(cid, ch) for cid in CONFIGS for ch in F.EDGE_CHANNELS[cid]]
TABLE = {}          # (label, family) -> [worst border ratio, worst interior ratio, n, calls]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n%-14s %-8s %12s %12s %6s %6s   err / (u S): border ring | interior; n = the bound" % ("kernel", "family", "border", "interior", "n", "calls"))
    print("(HEAD: S = the second layer's S_direct, n its own count; the bound asserted also carries the first layer's error, conv_float64.head64)")
    for (label, family), (border, inner, n, calls) in sorted(TABLE.items(), key=lambda kv: (kv[0][0], F.EDGE_FAMILIES.index(kv[0][1]))):
        print("%-14s %-8s %12.3f %12.3f %6d %6d" % (label, family, border, inner, n, calls))


def _worst(q, mask):
    return float(q[mask].max()) if mask.any() else 0.0


def _edge_check(got, family, x, w, b, val, Sd, stride, groups, ci_padded, tile, label, what, exact):
    """the bound, the exact zeros and the exact integers on one result; notes the border / interior ratios; returns the list of failures"""
    if got.shape != val.shape:
        return ["%s %s: shape %s, expected %s" % (what, family, got.shape, val.shape)]
    fails = []
    ring = np.broadcast_to(F.border_mask(val.shape[2], val.shape[3], *tile)[None, None], val.shape)
    leaky_b = F.round32_leaky(b, True)
    for c0, c1, alg, tag in groups:
        S = Sd[:, c0:c1] if alg == "direct" else F.S_wino(x, w[c0:c1], b[c0:c1], alg)
        g, v, r = got[:, c0:c1], val[:, c0:c1], ring[:, c0:c1]
        n = F.n_roundings(tag, ci_padded)
        err = np.abs(g.astype(np.float64) - v)
        err = np.where(np.isfinite(err), err, np.inf)
        over = err > F.bound(tag, ci_padded, S)
        q = np.where(S > 0, err / np.where(S > 0, F.U * S, 1.0), 0.0)
        row = TABLE.setdefault(("%s (%s)" % (label, alg) if len(groups) > 1 or label == "V1-1" else label, family), [0.0, 0.0, n, 0])
        row[0], row[1], row[2], row[3] = max(row[0], _worst(q, r)), max(row[1], _worst(q, ~r)), max(row[2], n), row[3] + 1
        if over.any():
            i = np.unravel_index(np.argmax(np.where(over, q, -1.0)), q.shape)
            fails.append("%s %s: %d outputs beyond n u S (%s, n = %d); worst %.2f u S at image %d channel %d pixel (%d, %d), %s" % (
                what, family, int(over.sum()), alg, n, float(q[i]), i[0], c0 + i[1], i[2], i[3], "border ring" if r[i] else "interior"))
        quiet = S == np.abs(b[c0:c1]).astype(np.float64)[None, :, None, None]          # every product zero
        if not np.array_equal(g[quiet], np.broadcast_to(leaky_b[None, c0:c1, None, None], g.shape)[quiet]):
            fails.append("%s %s: not exactly the bias where every product is zero" % (what, family))
    if family == "integers" and exact:
        want = F.round32_leaky(F.conv64(x, w, b, stride, False), True)
        if not np.array_equal(got, want):
            fails.append("%s integers: %d of %d outputs differ from the exact result" % (what, int((got != want).sum()), got.size))
    return fails


def _call(what, f):
    """a guard failure of the staging scope (or any error of the entry) fails the case at once, naming the shape; after a fault of the device
    nothing more is launched on it: the session ends"""
    try:
        return f()
    except B2FError as e:
        if any(s in str(e) for s in ("illegal memory access", "launch failure", "hardware exception")):
            pytest.exit("%s: %s -- the device faulted, no further launches" % (what, e), returncode=1)
        raise AssertionError("%s: %s" % (what, e)) from e


def test_every_kernel_of_the_table_has_a_case():
    swept = {cid for cid, _ in CASES}
    assert swept == set(CONFIGS) and set(F.GEOMETRY) == swept | {"HEAD", "F1"}
    assert {CONFIGS[cid][0] for cid in swept if cid not in EXPERIMENTS} == {"D1", "D2", "N2", "W2", "C16", "S16", "W4", "E1", "E2", "L2", "V1", "W6"}
    for cid in swept:
        assert F.EDGE_CHANNELS[cid] and F.edge_inputs(cid, CONFIGS[cid][1])
    wide = {co for _, co in F.EDGE_CHANNELS["W6"]}
    assert any(co % 64 == 0 for co in wide) and 32 in wide and any(co > 64 and 0 < co % 64 <= 32 for co in wide)


@pytest.mark.parametrize("cid,ch", CASES, ids=["%s-%dto%d" % ((cid,) + ch) for cid, ch in CASES])
def test_kernel_on_its_tile_and_block_edges(hard, cid, ch):
    tag, stride, _, opts, branches, exact = CONFIGS[cid]
    if cid in EXPERIMENTS and not hard.get_option("experiments"):
        pytest.skip("experiment kernel: not in the product library (python -m back2future_amd.build --experiments; B2F_LIB=back2future_amd/libb2f_exp.so)")
    ci, co = ch
    groups = _channel_groups(cid, co)
    expect = "W4" if (cid == "V1-1" and groups[0][2] == "F4") else tag
    tile = F.GEOMETRY[cid][:2]
    inputs = F.edge_inputs(cid, stride)
    fails, first, t0 = [], {}, time.time()
    with hard.options(**opts):           # (one option change per branch, not per shape: some of these options repack the model)
        for H, Wd, h, wd in inputs:
            for family in F.EDGE_FAMILIES:
                what = "%-9s %2d -> %3d %2dx%2d s%d" % (cid, ci, co, H, Wd, stride)
                x, w, b, val, Sd = F.edge_case(family, ci, co, H, Wd, stride)
                got, ran, cp = _call(what, lambda: _ran(hard, lambda: ops.conv3x3(hard, x, w, b, stride, True)))
                if ran != expect:
                    fails.append("%s %s: ran on %s, the case is meant for %s" % (what, family, ran, expect))
                    continue
                assert cp == F.padded(ci) and val.shape[2:] == (h, wd)
                if family == "gauss":
                    first[(H, Wd)] = got
                fails += _edge_check(got, family, x, w, b, val, Sd, stride, groups, cp, tile, cid, what, exact)
    for other in branches:
        with hard.options(**other):
            for (H, Wd), got in first.items():
                what = "%-9s %2d -> %3d %2dx%2d s%d %s" % (cid, ci, co, H, Wd, stride, other)
                x, w, b = F.make_case("gauss", F.SEED, F.BATCH, ci, co, H, Wd)
                again, ran2, _ = _call(what, lambda: _ran(hard, lambda: ops.conv3x3(hard, x, w, b, stride, True)))
                if ran2 != expect or not np.array_equal(again, got):
                    fails.append("%s: ran %s and gives %d other bits" % (what, ran2, int((again != got).sum())))
    print("%-9s %2d -> %3d: %d shapes x %d families, %d branches, %.1f s" % (cid, ci, co, len(inputs), len(F.EDGE_FAMILIES), len(branches), time.time() - t0))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails[:40])


def test_fused_head_on_its_strip_and_row_block_edges(hard):
    """ops.conv_head16 over the sweep of its stride-2 output (strips of 30 columns in 16-column tiles, row blocks above 16 rows), from odd and
    even inputs: inside head64's carried bound (head_measure), integers bit for bit"""
    fails = []
    tile = F.GEOMETRY["HEAD"][:2]
    for H, Wd, h, wd in F.edge_inputs("HEAD", 2):
        for family in F.EDGE_FAMILIES:
            what = "head 16 -> 16 -> 32 %2dx%2d" % (H, Wd)
            x, w1, b1, w2, b2 = F.head_case(family, H, Wd)
            got = _call(what, lambda: ops.conv_head16(hard, x, w1, b1, w2, b2))
            assert got.shape[2:] == (h, wd)
            r, _, r_bound, _ = F.head_measure(got, x, w1, b1, w2, b2)
            # head_measure asserts; this is the split of its first figure, err / (u S2), S2 the second layer's S_direct on the float64 map
            hidden = F.conv64(x, w1, b1, 1, True)
            S2 = F.S_direct(hidden, w2, b2, 2)
            err = np.abs(got.astype(np.float64) - F.conv64(hidden, w2, b2, 2, True))
            q = np.where(S2 > 0, np.where(np.isfinite(err), err, np.inf) / np.where(S2 > 0, F.U * S2, 1.0), 0.0)
            ring = np.broadcast_to(F.border_mask(h, wd, *tile)[None, None], q.shape)
            row = TABLE.setdefault(("HEAD", family), [0.0, 0.0, F.n_roundings("HEAD", 16), 0])
            row[0], row[1], row[3] = max(row[0], _worst(q, ring)), max(row[1], _worst(q, ~ring)), row[3] + 1
            if not r_bound <= 1.0:
                fails.append("%s %s: error is %.3f of the bound (%.2f u S2)" % (what, family, r_bound, r))
            if family == "integers":
                t = F.conv64(x, w1, b1, 1, False)
                assert t.min() >= 0
                want = F.round32_leaky(F.conv64(t, w2, b2, 2, False), True)
                if not np.array_equal(got, want):
                    fails.append("%s integers: %d of %d outputs differ from the exact result" % (what, int((got != want).sum()), got.size))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails[:40])


@pytest.mark.parametrize("normalize", [False, True])
def test_first_layer_on_its_block_edges(hard, normalize):
    """ops.conv_first (8 x 32 outputs per block) on the even maps it serves, with and without ColorNormalize: the bound of ROUNDINGS['F1'];
    integers without normalize bit for bit"""
    fails = []
    tile = F.GEOMETRY["F1"][:2]
    for H, Wd, h, wd in F.edge_inputs("F1", 2):
        for family in F.EDGE_FAMILIES:
            what = "first 3 -> 16 %2dx%2d s2%s" % (H, Wd, " normalized" if normalize else "")
            x9, w, b, x64 = F.first_case(family, (3, 16, H, Wd), normalize)
            got = _call(what, lambda: ops.conv_first(hard, x9, w, b, normalize))
            val, Sd = F.conv64(x64, w, b, 2, True), F.S_direct(x64, w, b, 2)
            assert val.shape[2:] == (h, wd)
            fails += _edge_check(got, family, x64, w, b, val, Sd, 2, [(0, 16, "direct", "F1")], 3, tile, "F1 norm" if normalize else "F1", what, not normalize)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails[:40])
