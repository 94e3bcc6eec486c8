"""CPU: the gradient of the Soft models' fine-tuning objective with respect to the output table (include/b2f.h, the *_grad_ft entries;
b2f_table_loss_grad_ft_host) without a GPU: (a) the host entry equals the numpy restatement of the definition bit for bit, (b) with both
flags 0 it gives the bits of b2f_table_loss_grad_host, (c) the restatement agrees with a float64 transcription of
SecondOrderSmoothnessCriterion.lua:77-104 and OBGCCriterion.lua:151-300 within one fp32 rounding plus a derived fp64 part, (d) the
transcription equals torch.autograd of the forward criteria where the specification is the derivative and differs where quirk 2 says
so, (e) malformed requests are refused with nothing written, (f) the symbols, the struct and the defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL
from tests import table_loss_grad_fields as TG
from tests import table_loss_grad_ft_fields as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_loss_grad_ft_defaults", "b2f_table_loss_grad_ft_host", "b2f_table_loss_grad_ft_device", "b2f_op_table_loss_grad_ft",
           "b2f_forward_loss_grad_ft", "b2f_forward_loss_grad_ft_device", "b2f_multi_forward_loss_grad_ft"]
# 1 x 1 .. 5 x 7: every border case of the radius-2 cross (no interior, one interior row / column, w < 3 with h >= 3 and the
# reverse); 3 x 9: three groups in an only interior row; 37 x 53: odd, several groups per row; (16,16,5): the coarsest levels are
# 2 x 2 and 1 x 1; (48,80,5): widths 80 .. 5
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (3, 9, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
OBJECTIVES = sorted(back2future.LOSS_OBJECTIVES)


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


def check_host(table, ref, past, flow_scale, o, what=""):
    got = ops.table_loss_grad(table, ref, flow_scale=flow_scale, options=TF.struct(o))
    want = TF.want_grad_ft(table, ref, past, flow_scale, o)
    assert len(got) == len(want) == len(table)
    for i, (g, w) in enumerate(zip(got, want)):
        same_bits(g, w, "%s tensor %d" % (what, i))
    return got


# ---- (f) symbols, struct, defaults ----

def test_symbols_struct_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in cdef and name + "(" in doc, name
    assert "b2f_loss_grad_ft_opts" in cdef and "b2f_loss_grad_ft_opts" in doc
    assert _lib.lib().b2f_version() >= 1008
    assert C.sizeof(_lib.LossGradOpts) == 104                              # unchanged
    assert C.sizeof(_lib.LossGradFtOpts) == 12 * 8 + 3 * 4 + 4 + 3 * 8     # 12 doubles, three ints, padding, three doubles
    o = back2future.loss_grad_ft_options()
    assert [getattr(o, k) for k in TF.TERMS] == [TG.DEFAULTS[k] for k in TF.TERMS]
    assert tuple(o.level_weights) == back2future.LOSS_LEVEL_WEIGHTS and o.size_average == 0
    assert (o.smooth_second_order, o.pme_criterion, o.pme_alpha, o.pme_beta, o.pme_gamma) == (1, 1, 1.0, 1.0, 1.0)
    k = back2future.loss_grad_ft_options(objective="Ours-Soft-ft-KITTI", size_average=True)
    assert (k.smooth_flow, k.pme, k.const_vel, k.smooth_occ, k.size_average) == (0.1, 2.0, 0.0001, 0.1, 1)
    assert (k.smooth_second_order, k.pme_criterion, k.pme_alpha, k.pme_beta, k.pme_gamma) == (1, 1, 0.0, 1.0, 1.0)
    s = back2future.loss_grad_ft_options(objective="Ours-Soft-ft-Sintel", pme_gamma=0.5, weights={"pme": 3.0})
    assert (s.pme, s.smooth_second_order, s.pme_criterion, s.pme_alpha, s.pme_beta, s.pme_gamma) == (3.0, 1, 1, 1.0, 0.0, 0.5)
    h = back2future.loss_grad_ft_options(objective="Ours-Hard")
    assert (h.smooth_flow, h.smooth_second_order, h.pme_criterion) == (2.0, 0, 0)
    for src in ("back2future_amd/csrc/b2f_tableloss_grad_ft.h", "back2future_amd/csrc/b2f_tableloss_grad_ft.hip"):
        text = open(os.path.join(ROOT, src)).read()
        assert "SecondOrderSmoothnessCriterion" in text and "OBGCC" in text, src
    with pytest.raises(ValueError, match="not provided"):                  # the first-order options keep refusing the Soft objectives
        back2future.loss_grad_options(objective="Ours-Soft-ft-KITTI")


# ---- (a) the host entry against the definition, bit for bit ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_entry_equals_the_definition(H, W, L, past):
    """wild and tame tables x flow_scale 20 and 10 x the three objectives x size_average, then each of the eight weights at 0"""
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        for scale in (20.0, 10.0):
            for name in OBJECTIVES:
                for avg in (False, True):
                    got = check_host(table, ref, past, scale, TF.objective(name, size_average=avg), "%s tame %d scale %g avg %d" % (name, tame, scale, avg))
        if not tame and H * W >= 64 * 64 // 2:
            assert any(np.isnan(g).any() for g in got) and all(np.isfinite(g).any() for g in got)      # NaN inputs reach the output, and stay local
        for k in TF.WEIGHTS8:
            check_host(table, ref, past, 20.0, TF.options(**{k: 0.0}), "%s = 0 tame %d" % (k, tame))


def test_alpha_alone_is_obcc():
    """OBGCC with alpha = 1, beta = gamma = 0 gives OBCC's bits; the objectives differ from one another"""
    table, ref = tables(48, 80, 5, True, False)
    a = ops.table_loss_grad(table, ref, options=TF.struct(TF.options(pme_beta=0.0, pme_gamma=0.0)))
    b = ops.table_loss_grad(table, ref, options=TF.struct(TF.options(pme_criterion="OBCC")))
    for i, (g, w) in enumerate(zip(a, b)):
        same_bits(g, w, "tensor %d" % i)
    c = ops.table_loss_grad(table, ref, options=TF.struct(TF.DEFAULTS))
    d = ops.table_loss_grad(table, ref, options=TF.struct(TF.options(smooth_second_order=False)))
    for j in range(5):
        assert not np.array_equal(a[5 * j + 3], c[5 * j + 3], equal_nan=True) and not np.array_equal(a[5 * j + 2], c[5 * j + 2], equal_nan=True)
        if j < 4:       # 3 x 5 has one interior row
            assert not np.array_equal(c[5 * j], d[5 * j], equal_nan=True) and not np.array_equal(c[5 * j + 1], d[5 * j + 1], equal_nan=True)
        np.testing.assert_array_equal(c[5 * j + 3], d[5 * j + 3])


def poke(table, i, b, c, y, x, v):
    """a copy of the table with one value replaced"""
    out = [t.copy() for t in table]
    out[i][b, c, y, x] = v
    return out


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_a_weight_of_zero_skips_its_term(past):
    """Each weight at 0 in turn: a NaN in the input of the switched-off term does not reach the elements that only that term would have
    spread it to -- which are NaN with the term on.  For beta and gamma that element is the warped image's gradient one pixel to the
    right of / below the NaN: it reads the poked pixel through ex(x - 1, y) or ey(x, y - 1) alone."""
    H, W, y, x = 16, 16, 8, 9
    table, ref = TL.tables(H, W, 2, past, tame=True)
    per = 5 if past else 4
    table = [t.copy() for t in table]
    for t in table[:per - 2]:       # the pixel and its surroundings: zero flows (targets inside), plain probabilities
        t[:, :, y - 3:y + 4, x - 3:x + 4] = np.float32(0.5) if t is table[per - 3] else np.float32(0)
    nan = np.float32(np.nan)
    i_o, i_iw1 = per - 3, per - 2
    # (term, the poked tensor / channel / pixel, the output tensor / channel / pixel that only this term makes NaN)
    cases = [("smooth_flow", (0, 0, y, x), (0, 0, y, x + 1)), ("smooth_flow", (0, 1, y, x), (0, 1, y - 1, x)),
             ("smooth_occ", (i_o, 0, y, x), (i_o, 0, y + 1, x)), ("prior_occ", (i_o, 1, y, x), (i_o, 0, y, x)),
             ("pme", (i_iw1, 2, y, x), (i_o, 1, y, x)),
             ("pme_beta", (i_iw1, 1, y, x), (i_iw1, 1, y, x + 1)), ("pme_gamma", (i_iw1, 1, y, x), (i_iw1, 1, y + 1, x))]
    if past:
        cases += [("const_vel", (0, 0, y, x), (1, 0, y, x)), ("smooth_flow", (1, 1, y, x), (1, 1, y - 1, x))]
    for term, (ti, tc, ty, tx), (gi, gc, gy, gx) in cases:
        bad = poke(table, ti, 0, tc, ty, tx, nan)
        got_off = check_host(bad, ref, past, 20.0, TF.options(**{term: 0.0}))
        got_on = check_host(bad, ref, past, 20.0, TF.DEFAULTS)
        assert np.isnan(got_on[gi][0, gc, gy, gx]), term
        assert np.isfinite(got_off[gi][0, gc, gy, gx]), term
        assert np.isfinite(got_off[gi][1]).all(), term                   # image 1 has no NaN at all
    # alpha: with beta = gamma = 0 too the photometric term has no addend left; the image gradient is +0.0, PO is +0.0 inside
    bad = poke(table, i_iw1, 0, 0, y, x, nan)
    got = check_host(bad, ref, past, 20.0, TF.options(pme_alpha=0.0, pme_beta=0.0, pme_gamma=0.0))
    assert not got[i_iw1].view(np.uint32).any() and np.isfinite(got[i_o]).all()
    got = check_host(bad, ref, past, 20.0, TF.options(pme_alpha=0.0))
    assert np.isnan(got[i_iw1][0, 0, y, x]) and np.isfinite(got[i_iw1][0, 1:]).all()       # beta and gamma still read it, in its channel
    g = ops.table_loss_grad(table, ref, options=TF.struct(TF.options(pme=0.0)))
    assert not g[per - 2].view(np.uint32).any() and not g[per - 1].view(np.uint32).any()
    if not past:        # a Hard table without the smoothness: its flow gradient is +0.0 everywhere
        g = ops.table_loss_grad(table, ref, options=TF.struct(TF.options(smooth_flow=0.0)))
        assert not g[0].view(np.uint32).any()


# ---- (b) both flags at 0: the first-order entry's bits ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_both_flags_off_is_the_first_order_entry(H, W, L, past):
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        for avg in (False, True):
            o = TF.options(smooth_second_order=False, pme_criterion="OBCC", pme_alpha=0.0, pme_beta=7.0, pme_gamma=0.25, size_average=avg)
            got = ops.table_loss_grad(table, ref, options=TF.struct(o))
            first = ops.table_loss_grad(table, ref, options=TG.struct(TF.first_order(o)))
            for i, (g, w) in enumerate(zip(got, first)):
                same_bits(g, w, "tensor %d" % i)


# ---- (c) the definition against the reference's updateGradInput functions ----

@pytest.mark.parametrize("variant", ["default", "size_average", "Ours-Soft-ft-KITTI", "Ours-Soft-ft-Sintel"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)])
def test_definition_against_the_lua_gradients(H, W, L, past, variant):
    """Per element |want - lua| <= 2^-24 |v| + 2^-149 + 2^-48 m + 2^-50 mt, m the sum of the magnitudes of the element's terms and mt
    the same sum over the terms that carry a contrast weight E(t), each scaled by 1 + |t| / 2.  Derivation, as for the first-order
    table: `want` is the fp64 sum rounded to fp32 once -- half an ulp, 2^-24 |v| for a normal v, at most 2^-149 for a subnormal one.
    Before the rounding the two sides differ (1) in the exponential, loss_exp against np.exp: 2^-50 relative
    (test_exponential_against_numpy of tests/test_table_loss_cpu.py); (2) in the rounding of its argument, -20 * (a / 3 + b / 3)
    against -20 * (mean + mean): at most four roundings of 2^-53 |t| in t, so 2^-51 |t| relative in the weight -- together 2^-50 (1 +
    |t| / 2) of every weighted term; (3) in the other fp64 roundings on the way of a term into the element.  The longest way is that
    of an OBGCC image term: D1 (a square, an add, a root or a power, a division: 4), times alpha, beta or gamma (1), four adds (4),
    times o (1), the coefficient (three products and a division: 4), times it (1): 15 on each side, each at most 2^-53 of the sum of
    the magnitudes; a second-order term has 4 + 1 (the weight) + 5 (adds) + 3 + 1 = 14.  30 roundings of 2^-53 are less than 2^-48.
    Nothing is tuned."""
    table, ref = tables(H, W, L, past, True)
    o = TF.objective(variant) if variant in back2future.LOSS_OBJECTIVES else TF.options(size_average=variant == "size_average")
    want, mag, want64 = TF.want_grad_ft(table, ref, past, o=o, with_mag=True)
    lua = TF.lua_grad_ft(table, ref, past, o=o)
    worst = worst64 = 0.0
    for i, (w, (m, mt), w64, l) in enumerate(zip(want, mag, want64, lua)):
        assert np.isfinite(w).all() and np.isfinite(l).all()
        part64 = 2.0 ** -48 * m + 2.0 ** -50 * mt
        bar = 2.0 ** -24 * np.abs(l) + 2.0 ** -149 + part64
        frac = float((np.abs(w.astype(np.float64) - l) / bar).max())
        worst = max(worst, frac)
        worst64 = max(worst64, float((np.abs(w64 - l) / (part64 + 2.0 ** -149)).max()))
        assert frac <= 1.0, (i, frac)
    assert sum(float(np.abs(l).max()) > 0 for l in lua) >= len(lua) - 2 * L - 2         # (a tiny level: every target may leave, no interior)
    print("H %d W %d L %d past %d %s: largest fraction of the bar %.3f; before the rounding, of its fp64 part %.3f" % (H, W, L, past, variant, worst, worst64))


# ---- (d) the reference's gradients against torch.autograd of its forward criteria ----

def _autograd(table, ref, past, o):
    import torch
    tens = [torch.tensor(t.astype(np.float64), requires_grad=True) for t in table]
    TF.torch_terms(tens, ref, past, o=o).backward()
    return [t.grad.numpy() if t.grad is not None else np.zeros(t.shape) for t in tens]


def _only(o, **kw):
    """the options with every term off but those named"""
    z = dict((k, 0.0) for k in TF.TERMS)
    z.update(kw)
    return TF.options(**dict(o, **z))


@pytest.mark.parametrize("size_average", [False, True], ids=["sum", "size_average"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_second_order_gradient_is_the_derivative(past, size_average):
    """On f and p the transcription of SecondOrderSmoothnessCriterion.lua:77-104 equals autograd of lines 28-75 everywhere.  The bar:
    64 fp64 roundings of the element's magnitude (each side is a sum of six products of a few operations)."""
    H, W, L = 48, 80, 5
    table, ref = tables(H, W, L, past, True)
    per = 5 if past else 4
    o = _only(TF.options(size_average=size_average), smooth_flow=1.0)
    lua = TF.lua_grad_ft(table, ref, past, o=o)
    auto = _autograd(table, ref, past, o)
    for j in range(L):
        for i in range(2 if past else 1):
            got, a = lua[j * per + i], auto[j * per + i]
            assert j > 0 or float(np.abs(got).max()) > 0          # (the flows of the coarse levels are too plain for a second difference)
            np.testing.assert_allclose(got, a, rtol=0, atol=64.0 * 2.0 ** -53 * max(1.0, float(np.abs(got).max())), err_msg="level %d tensor %d" % (j, i))


def _flat_occlusions(table, per, inside=True, seed=0):
    """the table with zero flows (every target inside) and occlusion planes constant per image"""
    out = [t.copy() for t in table]
    r = np.random.default_rng(seed)
    for j in range(len(table) // per):
        for i in range(per - 3):
            out[j * per + i][...] = 0
        oc = out[j * per + per - 3]
        oc[...] = r.uniform(0.2, 0.9, (oc.shape[0], 2, 1, 1)).astype(np.float32)
    return out


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_obgcc_image_gradient_is_the_derivative_under_flat_occlusions(past):
    """Occlusion planes constant per image, all targets inside, alpha = 1: the transcription of OBGCCriterion.lua:151-300 equals
    autograd of lines 39-149 on both warped images.  With varying occlusions it does not: the neighbour's share is weighted with the
    pixel's own o (quirk 2), and the difference is exactly o(x,y) - o of the neighbour times that share.  The bar: 64 fp64 roundings
    of the element's magnitude."""
    H, W, L = 48, 80, 5
    table, ref = tables(H, W, L, past, True)
    per = 5 if past else 4
    o = _only(TF.options(pme_beta=0.75, pme_gamma=1.5), pme=1.0)
    flat = _flat_occlusions(table, per)
    lua = TF.lua_grad_ft(flat, ref, past, o=o)
    auto = _autograd(flat, ref, past, o)
    for j in range(L):
        for i in (per - 2, per - 1):
            got, a = lua[j * per + i], auto[j * per + i]
            assert float(np.abs(got).max()) > 0
            np.testing.assert_allclose(got, a, rtol=0, atol=64.0 * 2.0 ** -53 * max(1.0, float(np.abs(got).max())), err_msg="level %d tensor %d" % (j, i))
    # varying occlusions, still all inside
    vary = [t.copy() for t in flat]
    for j in range(L):
        vary[j * per + per - 3][...] = table[j * per + per - 3]
    assert float(np.ptp(vary[per - 3][0, 0])) > 0.1
    lua = TF.lua_grad_ft(vary, ref, past, o=o)
    auto = _autograd(vary, ref, past, o)
    for i in (per - 2, per - 1):
        gap = np.abs(lua[i] - auto[i])
        assert float(gap.max()) > 1e-6 * float(np.abs(lua[i]).max()) and float(gap.max()) > 1e4 * 2.0 ** -53, i


# ---- (e) argument errors, each with nothing written ----

def _call_host(table, ref, grad, past, opts=None, n_outs=None, H=None, W=None):
    n = ref.shape[0]
    tp = (_lib.c_float_p * len(table))(*[_lib.fptr(t) for t in table])
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
    return _lib.lib().b2f_table_loss_grad_ft_host(tp, len(table) if n_outs is None else n_outs, n, H or ref.shape[2], W or ref.shape[3], int(past),
                                                  _lib.fptr(ref), 20.0, C.byref(opts) if opts is not None else None, gp)


def test_malformed_requests_are_refused_with_nothing_written():
    table, ref = TL.tables(16, 16, 2, False, tame=True)
    grad = [np.full(t.shape, 7.0, np.float32) for t in table]

    def refused(rc, match):
        with pytest.raises(_lib.B2FError, match=match):
            _lib.check(rc)
        assert all((g == 7.0).all() for g in grad)

    assert _call_host(table, ref, grad, False) == 0 and not any((g == 7.0).all() for g in grad)
    want = TF.want_grad_ft(table, ref, False)                                                  # opts = NULL: the defaults
    for g, w in zip(grad, want):
        same_bits(g, w)
    for g in grad:
        g[...] = 7.0
    before = [t.copy() for t in table] + [ref.copy()]
    refused(_call_host(table, ref, [table[0]] + grad[1:], False), "alias")                    # an output is a tensor of the table
    refused(_call_host(table, ref, grad[:3] + [table[6]] + grad[4:], False), "alias")         # ... of another level
    refused(_call_host(table, ref, grad[:7] + [ref], False), "alias")   # ... ref
    refused(_call_host(table, ref, [grad[1]] + grad[1:], False), "alias")                     # two outputs share a buffer
    for t, b in zip(table + [ref], before):
        np.testing.assert_array_equal(t, b)
    for field, value in (("pme", -1.0), ("smooth_occ", float("nan")), ("const_vel", float("inf")), ("pme_alpha", -0.5), ("pme_beta", float("nan")),
                         ("pme_gamma", float("inf"))):
        o = back2future.loss_grad_ft_options()
        setattr(o, field, value)
        refused(_call_host(table, ref, grad, False, opts=o), "finite and >= 0")
    o = back2future.loss_grad_ft_options()
    o.level_weights[6] = -0.5
    refused(_call_host(table, ref, grad, False, opts=o), "finite and >= 0")
    for value in (2, -1):
        o = back2future.loss_grad_ft_options()
        o.pme_criterion = value
        refused(_call_host(table, ref, grad, False, opts=o), "pme_criterion")
    refused(_call_host(table, ref, grad, True), "n_outs")                                      # 8 tensors are no Soft table
    refused(_call_host(table[:7], ref, grad[:7], False), "n_outs")
    big = [np.zeros((1, 3 if i % 4 >= 2 else 2, 128 >> (i // 4), 128 >> (i // 4)), np.float32) for i in range(32)]
    out = [np.full(t.shape, 7.0, np.float32) for t in big]
    with pytest.raises(_lib.B2FError, match="1 .. 7 levels"):
        _lib.check(_call_host(big, np.zeros((1, 3, 128, 128), np.float32), out, False))
    assert all((g == 7.0).all() for g in out)
    with pytest.raises(ValueError, match="finite and >= 0"):
        back2future.loss_grad_ft_options(weights={"pme": -2.0})
    with pytest.raises(ValueError, match="finite and >= 0"):
        back2future.loss_grad_ft_options(pme_beta=-1.0)
    with pytest.raises(ValueError, match="unknown weight"):
        back2future.loss_grad_ft_options(weights={"entropy": 1.0})
    with pytest.raises(ValueError, match="OBCC"):
        back2future.loss_grad_ft_options(pme_criterion="SSIM")
    with pytest.raises(ValueError, match="unknown objective"):
        back2future.loss_grad_ft_options(objective="Ours-Medium")
    with pytest.raises(ValueError, match="loss_grad_options or loss_grad_ft_options"):
        ops.table_loss_grad(table, ref, options={"pme": 1.0})
