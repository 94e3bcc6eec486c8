"""CPU: the gradient table with the occlusion-aware SSIM + L1 photometric term (include/b2f.h, the *_grad_ssim entries;
b2f_table_loss_grad_ssim_host) without a GPU: (a) the host entry equals the numpy restatement of the definition bit for bit, (b) with
pme = 0 it gives the bits of b2f_table_loss_grad_ft_host, and its flow planes always, (c) the restatement agrees with a float64
transcription of OSSIML1Criterion.lua:165-302 within one fp32 rounding plus a derived fp64 part, (d) the transcription equals
torch.autograd of the pixel's own window term at interior pixels and differs where the quirks say so, (e) wrong readings of the
definition are told from it, (f) malformed requests are refused with nothing written, (g) the symbols, the struct and the defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL
from tests import table_loss_grad_ft_fields as TF
from tests import table_loss_grad_ssim as TGS
from tests import table_loss_ssim_fields as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_loss_grad_ssim_defaults", "b2f_table_loss_grad_ssim_host", "b2f_table_loss_grad_ssim_device", "b2f_op_table_loss_grad_ssim",
           "b2f_forward_loss_grad_ssim", "b2f_forward_loss_grad_ssim_device", "b2f_multi_forward_loss_grad_ssim"]
# 1 x 1 .. 5 x 7: every border case of the 3 x 3 window and of the five-point cross; 37 x 53: odd, several groups per row;
# (16,16,5): the coarsest levels are 2 x 2 and 1 x 1; (48,80,5): widths 80 .. 5
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
ALPHAS = (1.0, 0.85, 0.5, 0.0)


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


_TABLES = {}


def tables(H, W, L, past, tame):
    key = (H, W, L, past, tame)
    if key not in _TABLES:
        _TABLES[key] = TL.tables(H, W, L, past, tame=tame)
    return _TABLES[key]


def same_bits(got, want, what=""):
    """float32 arrays equal bit for bit; two NaNs in the same place count as equal"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = (g != w) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d elements differ, first at %r: got %r want %r" % (what, bad.sum(), tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def wide_ranges(L):
    """a given range per level that does not hold the values: normalised values leave [0, 1]"""
    return np.array([[-0.25 - 0.125 * j, 0.75 + 0.0625 * j] for j in range(L)], np.float32)


def host(table, ref, flow_scale, o, mode, ranges):
    return ops.table_loss_grad(table, ref, flow_scale=flow_scale, options=TGS.struct(o), ssim_range=TGS.range_arg(mode, ranges))


def check_host(table, ref, past, flow_scale, o, mode=TGS.BATCH, ranges=None, what=""):
    got = host(table, ref, flow_scale, o, mode, ranges)
    want = TGS.want_grad_ssim(table, ref, past, flow_scale, o, mode, ranges)
    assert len(got) == len(want) == len(table)
    for i, (g, w) in enumerate(zip(got, want)):
        same_bits(g, w, "%s tensor %d" % (what, i))
    return got


# ---- (g) symbols, struct, defaults ----

def test_symbols_struct_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in doc, name
    assert _lib.lib().b2f_version() >= 1011
    assert C.sizeof(_lib.LossGradOpts) == 104 and C.sizeof(_lib.LossGradFtOpts) == 136      # unchanged
    assert C.sizeof(_lib.LossGradSsimOpts) == 12 * 8 + 2 * 4 + 8                            # 12 doubles, two ints, alpha
    o = back2future.loss_grad_ssim_options()
    d = back2future.loss_grad_options()
    assert [getattr(o, k) for k in TGS.TERMS] == [getattr(d, k) for k in TGS.TERMS]
    assert tuple(o.level_weights) == back2future.LOSS_LEVEL_WEIGHTS and o.size_average == 0
    assert (o.smooth_second_order, o.ssim_alpha) == (0, 0.85)
    s = back2future.loss_grad_ssim_options(pme_criterion="OSSIM", smooth_second_order=True, size_average=True, weights={"pme": 3.0})
    assert (s.ssim_alpha, s.smooth_second_order, s.size_average, s.pme) == (1.0, 1, 1, 3.0)
    assert back2future.loss_grad_ssim_options(pme_criterion="OSSIM", ssim_alpha=0.25).ssim_alpha == 0.25
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            back2future.loss_grad_ssim_options(ssim_alpha=bad)
    with pytest.raises(ValueError):
        back2future.loss_grad_ssim_options(pme_criterion="OBCC")
    for src in ("back2future_amd/csrc/b2f_tableloss_grad_ssim.h", "back2future_amd/csrc/b2f_tableloss_grad_ssim.hip"):
        assert "OSSIML1Criterion.lua:165-302" in open(os.path.join(ROOT, src)).read(), src


# ---- (a) the host entry against the definition, bit for bit ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_entry_equals_the_definition(H, W, L, past):
    """wild and tame tables x flow_scale 20 and 10 x the three range modes and a given range that does not hold the values x four alphas
    x second order x size_average, then each weight at 0"""
    given = np.array([[-3.0, 3.0]] * L, np.float32)
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        for scale in (20.0, 10.0):
            for i, alpha in enumerate(ALPHAS):
                second, avg = bool(i & 1), bool(i & 2)
                o = TGS.options(ssim_alpha=alpha, smooth_second_order=second, size_average=avg)
                for mode, ranges in ((TGS.BATCH, None), (TGS.IMAGE, None), (TGS.GIVEN, given), (TGS.GIVEN, wide_ranges(L))):
                    if scale == 10.0 and mode != TGS.BATCH:
                        continue
                    check_host(table, ref, past, scale, o, mode, ranges, "tame %d scale %g alpha %g mode %d" % (tame, scale, alpha, mode))
        check_host(table, ref, past, 20.0, TGS.options(smooth_second_order=True, size_average=True), TGS.IMAGE, None, "second + avg")
        for k in TGS.TERMS:
            check_host(table, ref, past, 20.0, TGS.options(**{k: 0.0}), TGS.IMAGE, None, "%s = 0 tame %d" % (k, tame))


def test_a_switched_off_term_is_not_evaluated():
    """pme = 0: a NaN in a warped image, which only the photometric term reads, stays out of the whole table (the range is not
    computed from it either: NaNs are skipped); with the term on it reaches that image's gradient and the occlusions'"""
    table, ref = tables(5, 7, 1, True, True)
    poked = [t.copy() for t in table]
    poked[3][0, 1, 2, 3] = np.nan
    off = host(poked, ref, 20.0, TGS.options(pme=0.0), TGS.BATCH, None)
    assert all(np.isfinite(g).all() for g in off)
    assert not off[3].any() and not off[4].any()
    on = host(poked, ref, 20.0, TGS.options(), TGS.GIVEN, np.array([[-3.0, 3.0]], np.float32))
    assert np.isnan(on[3][0, 1]).any() and np.isfinite(on[3][0, 0]).all() and np.isfinite(on[4]).all() and np.isfinite(on[3][1]).all()
    check_host(poked, ref, True, 20.0, TGS.options(), TGS.BATCH, None, "poked")


def test_an_unusable_range_follows_ieee():
    """a zero span: NaN or Inf in the elements inside the image that read the range, +0.0 / k_p outside, as the restatement gives"""
    table, ref = tables(5, 7, 1, False, True)
    zero = np.array([[0.5, 0.5]], np.float32)
    got = host(table, ref, 20.0, TGS.options(), TGS.GIVEN, zero)
    want = TGS.want_grad_ssim(table, ref, False, 20.0, TGS.options(), TGS.GIVEN, zero)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.isfinite(g), np.isfinite(w))
        np.testing.assert_array_equal(g[np.isfinite(g)], w[np.isfinite(w)])
    assert not np.isfinite(got[2]).all() and np.isfinite(got[0]).all()


# ---- (b) against the existing entries ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_without_pme_it_is_the_fine_tuning_entry(past):
    table, ref = tables(48, 80, 5, past, False)
    for second in (False, True):
        o = TGS.options(pme=0.0, smooth_second_order=second)
        a = host(table, ref, 20.0, o, TGS.IMAGE, None)
        b = ops.table_loss_grad(table, ref, options=TF.struct(TGS.ft_options(o)))
        for i, (g, w) in enumerate(zip(a, b)):
            same_bits(g, w, "pme 0 tensor %d" % i)
        o = TGS.options(pme=2.0, smooth_second_order=second, ssim_alpha=0.5)
        a = host(table, ref, 20.0, o, TGS.BATCH, None)
        b = ops.table_loss_grad(table, ref, options=TF.struct(TGS.ft_options(o)))
        per = 5 if past else 4
        for j in range(5):
            for i in range(per - 3):
                same_bits(a[j * per + i], b[j * per + i], "flow plane %d of level %d" % (i, j))
            assert not np.array_equal(a[j * per + per - 2], b[j * per + per - 2], equal_nan=True)


# ---- (e) wrong readings of the definition ----

@pytest.mark.parametrize("mutation", TGS.MUTATIONS)
@pytest.mark.parametrize("H,W", [(1, 5), (3, 3)])
def test_a_wrong_reading_is_told_from_the_definition(H, W, mutation):
    table, ref = tables(H, W, 1, True, True)
    o = TGS.options()
    got = host(table, ref, 20.0, o, TGS.BATCH, None)
    wrong = TGS.want_grad_ssim(table, ref, True, 20.0, o, TGS.BATCH, None, mutation=mutation)
    assert any(not np.array_equal(g, w, equal_nan=True) for g, w in zip(got, wrong)), mutation


# ---- (f) refusals: nothing is written ----

def test_refusals_write_nothing():
    table, ref = tables(16, 16, 5, True, True)
    n, H, W = ref.shape[0], 16, 16
    lib = _lib.lib()
    grad = [np.full(t.shape, 7.0, np.float32) for t in table]
    ptrs = (_lib.c_float_p * len(table))(*[_lib.fptr(t) for t in table])
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])

    def call(opts=None, n_outs=len(table), g=gp, mode=TGS.IMAGE, ranges=None, tab=ptrs):
        return lib.b2f_table_loss_grad_ssim_host(tab, n_outs, n, H, W, 1, _lib.fptr(ref), 20.0, C.byref(opts) if opts is not None else None, g, mode, ranges)

    def refused(rc, what):
        assert rc != 0, what
        assert all((x == 7.0).all() for x in grad), what + ": written"

    assert call() == 0 and not any((x == 7.0).all() for x in grad)
    for x in grad:
        x.fill(7.0)
    aliased = (_lib.c_float_p * len(grad))(*([_lib.fptr(table[0])] + [_lib.fptr(g) for g in grad[1:]]))
    refused(call(g=aliased), "aliases the table")
    twice = (_lib.c_float_p * len(grad))(*([_lib.fptr(grad[1])] + [_lib.fptr(g) for g in grad[1:]]))
    refused(call(g=twice), "aliases itself")
    for field, bad in (("pme", -1.0), ("smooth_occ", float("inf")), ("prior_occ", float("nan")), ("ssim_alpha", -0.01), ("ssim_alpha", 1.01),
                       ("ssim_alpha", float("nan"))):
        o = back2future.loss_grad_ssim_options()
        setattr(o, field, bad)
        refused(call(opts=o), "%s = %r" % (field, bad))
    o = back2future.loss_grad_ssim_options()
    o.level_weights[2] = -0.5
    refused(call(opts=o), "level weight")
    refused(call(mode=3), "range_mode 3")
    refused(call(mode=-1), "range_mode -1")
    refused(call(mode=TGS.GIVEN, ranges=None), "given without ranges")
    refused(call(n_outs=len(table) - 1), "n_outs")
    refused(call(n_outs=0), "n_outs 0")
    # L > 7: eight levels of a Hard table
    big = [np.zeros((1, 2 if i % 4 < 2 else 3, 128 >> (i // 4), 128 >> (i // 4)), np.float32) for i in range(32)]
    bg = [np.full(t.shape, 7.0, np.float32) for t in big]
    rc = lib.b2f_table_loss_grad_ssim_host((_lib.c_float_p * 32)(*[_lib.fptr(t) for t in big]), 32, 1, 128, 128, 0,
                                           _lib.fptr(np.zeros((1, 3, 128, 128), np.float32)), 20.0, None,
                                           (_lib.c_float_p * 32)(*[_lib.fptr(g) for g in bg]), TGS.IMAGE, None)
    assert rc != 0 and all((x == 7.0).all() for x in bg)
    with pytest.raises(ValueError):
        ops.table_loss_grad(table, ref, options=back2future.loss_grad_ssim_options(), ssim_range="neither")
    with pytest.raises(ValueError):
        ops.table_loss_grad(table, ref, options=back2future.loss_grad_ssim_options(), ssim_range=np.zeros((4, 2), np.float32))


# ---- (c) the restatement against the transcription of the Lua ----

_SHARE = {}


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("alpha", [1.0, 0.85, 0.0])
def test_restatement_agrees_with_the_lua(past, alpha):
    """per element within 2^-24 |v| + 2^-149 + a m, a = allowance_ssim_grad() (derived there), m the sum of the magnitudes of the
    element's terms; tame tables (finite values), the batch range, which holds the values"""
    a = TGS.allowance_ssim_grad()
    worst = 0.0
    for (H, W, L) in ((5, 7, 1), (37, 53, 1), (48, 80, 5)):
        table, ref = tables(H, W, L, past, True)
        for second, avg in ((False, False), (True, True)):
            o = TGS.options(ssim_alpha=alpha, smooth_second_order=second, size_average=avg)
            want, mags, sums = TGS.want_grad_ssim(table, ref, past, 20.0, o, TGS.BATCH, None, with_mag=True)
            lua = TGS.lua_grad_ssim(table, ref, past, 20.0, o)
            per = 5 if past else 4
            for i, (w, l, m, s64) in enumerate(zip(want, lua, mags, sums)):
                if m is None:       # the flow planes: tests/test_table_loss_grad_ft_cpu.py holds them
                    continue
                v = np.abs(l)
                bar = 2.0 ** -24 * v + 2.0 ** -149 + a * m
                err = np.abs(w.astype(np.float64) - l)
                # the fp64 sums before the one rounding are held to the fp64 part alone, which is what `a` was derived for
                share = (np.abs(s64 - l) / (a * m + 1e-300)).max()
                worst = max(worst, float(share))
                assert share <= 1.0 and (err <= bar).all(), "tensor %d of %d x %d: share of the fp64 part %g" % (i, H, W, share)
    _SHARE[(past, alpha)] = worst
    print("largest share of a m used: %.3g" % worst)


# ---- (d) the transcription against torch.autograd ----

def _own_window_terms(x, y, occ, alpha, rng):
    """o (alpha (1 - l cs) + (1 - alpha) P1(x - y)) per pixel and channel in torch float64 on values normalised by rng: the forward value
    of line 119, kept per pixel"""
    import torch
    import torch.nn.functional as F
    weight = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
    for c in range(3):
        weight[c, c] = torch.from_numpy(TS.gaussian3())
    conv = lambda a: F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), weight)
    mn, mx = rng
    xn, yn = (x - mn) / (mx - mn), (y - mn) / (mx - mn)
    mu_x, mu_y = conv(xn), conv(yn)
    s_x, s_y, s_xy = conv(xn * xn) - mu_x ** 2, conv(yn * yn) - mu_y ** 2, conv(xn * yn) - mu_x * mu_y
    l = (2 * mu_x * mu_y + TS.C1) / (mu_x ** 2 + mu_y ** 2 + TS.C1)
    cs = (2 * s_xy + TS.C2) / (s_x + s_y + TS.C2)
    d = xn - yn
    gw = float(TS.gaussian3()[1, 1])
    # the magnitudes of the terms of the derivative with respect to x: l and cs counted as 1, a difference as the sum of its operands
    mag = occ.abs() * (alpha * (2 * gw * (mu_y + mu_x).abs() / (mu_x ** 2 + mu_y ** 2 + TS.C1) +
                                2 * gw * (yn.abs() + mu_y.abs() + xn.abs() + mu_x.abs()) / (s_x + s_y + TS.C2)) +
                       (1 - alpha) * (d / torch.sqrt(d * d + 1e-6)).abs()) / (mx - mn)
    return occ * (alpha * (1 - l * cs) + (1 - alpha) * torch.sqrt(d * d + 1e-6)), mag.detach().numpy()


@pytest.mark.parametrize("alpha", [1.0, 0.85])
def test_transcription_is_the_own_window_diagonal(alpha):
    """zero flows (every target inside), 48 x 80, given range (0, 1).  For each of the nine offsets of a stride-3 lattice the per-pixel
    terms are summed over the lattice, whose windows do not overlap, and differentiated: the gradient at the lattice's pixels is the
    diagonal of the Jacobian of the pixel's own window term.  At interior pixels updateGradInput's image gradient equals it within 64
    fp64 roundings of the terms' magnitudes (quirk 1 is all that separates it from the full derivative); on the border it does not
    (quirk 2).  The occlusion gradient is the forward pixel value.  With range (0, 2) the two differ by the factor of quirk 3."""
    import torch
    H, W = 48, 80
    table, ref = tables(H, W, 1, False, True)
    table = [t.copy() for t in table]
    table[0][:] = 0.0
    sub = [t[:1] for t in table]
    target = ref[:1]
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    interior = (iy > 0) & (iy < H - 1) & (ix > 0) & (ix < W - 1)
    for mn, mx in ((0.0, 1.0), (0.0, 2.0)):
        back = TGS.ossiml1_back(sub, target, False, 20.0, alpha, mn, mx, False)
        for d in range(2):
            occ = torch.from_numpy(sub[1][:, 1 - d:2 - d].astype(np.float64))
            y = torch.from_numpy(target.astype(np.float64))
            x = torch.from_numpy(sub[2 + d].astype(np.float64)).requires_grad_(True)
            terms, scale = _own_window_terms(x, y, occ, alpha, (mn, mx))
            diag = np.zeros((1, 3, H, W))
            for oy in range(3):
                for ox in range(3):
                    (g,) = torch.autograd.grad(terms[:, :, oy::3, ox::3].sum(), x, retain_graph=True)
                    diag[:, :, oy::3, ox::3] = g.numpy()[:, :, oy::3, ox::3]
            lua = back[1 + d] * 6.0 / (mx - mn)        # line 289's 1 / 6 undone; quirk 3: the Lua lacks 1 / (mx - mn)
            err = np.abs(lua - diag)
            share = (err[:, :, interior] / (64 * 2.0 ** -53 * scale[:, :, interior] + 1e-300)).max()
            print("alpha %g range (%g, %g) direction %d: share of 64 roundings used %.3g" % (alpha, mn, mx, d, share))
            assert share <= 1.0
            assert (err[:, :, ~interior] > 1e-6).any()                                              # quirk 2
            if mx - mn != 1.0:
                assert np.abs(back[1 + d] * 6.0 - diag)[:, :, interior].max() > 1e-6                # quirk 3
            # the occlusion gradient is the forward pixel value before the occlusion weight (every target is inside)
            fwd = _own_window_terms(x.detach(), y, torch.ones_like(occ), alpha, (mn, mx))[0].sum(1).numpy()
            np.testing.assert_allclose(back[0][:, 1 - d] * 6.0, fwd, rtol=1e-12, atol=1e-15)
