"""CPU: the gradient of the pme objective with respect to the output table (`gradOutputs` of train.lua:428-468; include/b2f.h,
b2f_table_loss_grad_host) without a GPU: (a) the host entry equals the numpy restatement of the definition bit for bit, (b) the
restatement agrees with a float64 transcription of the reference's updateGradInput functions within one fp32 rounding plus the
exponential's error, (c) the transcription differs from torch.autograd of the forward criteria by exactly the two documented constants
on the occlusions and by nothing elsewhere, (d) malformed requests are refused with nothing written."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL
from tests import table_loss_grad_fields as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_loss_grad_defaults", "b2f_table_loss_grad_host", "b2f_table_loss_grad_device", "b2f_op_table_loss_grad", "b2f_forward_loss_grad",
           "b2f_forward_loss_grad_device", "b2f_multi_forward_loss_grad"]
# 1 x 1 .. 5 x 7: every border case of the cross; 37 x 53: odd, several groups per row; (16,16,5): the coarsest level is 1 x 1;
# (48,80,5): widths 80 .. 5
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
OTHER = {"smooth_flow": 2.0, "const_vel": 0.25, "pme": 3.0, "smooth_occ": 0.5, "prior_occ": 0.0625,
         "level_weights": (0.5, 0.25, 1.0, 0.125, 2.0, 0.64, 1.28)}


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


def check_host(table, ref, past, flow_scale, o):
    got = ops.table_loss_grad(table, ref, flow_scale=flow_scale, options=TG.struct(o))
    want = TG.want_grad(table, ref, past, flow_scale, o)
    assert len(got) == len(want) == len(table)
    for i, (g, w) in enumerate(zip(got, want)):
        same_bits(g, w, "tensor %d" % i)
    return got


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
    assert "b2f_loss_grad_opts" in cdef and "b2f_loss_grad_opts" in doc
    assert _lib.lib().b2f_version() >= 1007
    o = back2future.loss_grad_options()
    assert [getattr(o, k) for k in TG.TERMS] == [back2future.LOSS_WEIGHTS[k] for k in TG.TERMS] == [TG.DEFAULTS[k] for k in TG.TERMS]
    assert tuple(o.level_weights) == back2future.LOSS_LEVEL_WEIGHTS == TG.DEFAULTS["level_weights"] and o.size_average == 0
    assert C.sizeof(_lib.LossGradOpts) == 5 * 8 + 7 * 8 + 8          # the C struct: 12 doubles, an int, padding
    hard = back2future.loss_grad_options(objective="Ours-Hard", size_average=True)
    assert (hard.smooth_flow, hard.pme, hard.const_vel, hard.size_average) == (2.0, 1.0, 1.0, 1)
    for src in ("back2future_amd/csrc/b2f_tableloss_grad.h", "back2future_amd/csrc/b2f_tableloss_grad.hip"):
        assert "train.lua:428-468" in open(os.path.join(ROOT, src)).read(), src


# ---- (a) the host entry against the definition, bit for bit ----

@pytest.mark.parametrize("tame", [False, True], ids=["wild", "tame"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_entry_equals_the_definition(H, W, L, past, tame):
    table, ref = tables(H, W, L, past, tame)
    got = check_host(table, ref, past, 20.0, TG.DEFAULTS)
    if not tame and H * W >= 64 * 64 // 2:
        assert any(np.isnan(g).any() for g in got) and all(np.isfinite(g).any() for g in got)      # NaN inputs reach the output, and stay local


@pytest.mark.parametrize("variant", ["scale10", "weights", "size_average", "weights_size_average_scale10"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (37, 53, 1), (48, 80, 5)])
def test_host_entry_with_other_options(H, W, L, past, variant):
    table, ref = tables(H, W, L, past, False)
    o = TG.options(**(OTHER if "weights" in variant else {}))
    o["size_average"] = "size_average" in variant
    got = check_host(table, ref, past, 10.0 if "scale10" in variant else 20.0, o)
    if L > 1:       # the option changes something (at 5 x 7 the targets of both scales leave the image alike)
        base = ops.table_loss_grad(table, ref)
        assert any(not np.array_equal(g, b, equal_nan=True) for g, b in zip(got, base))


def poke(table, i, b, c, y, x, v):
    """a copy of the table with one value replaced"""
    out = [t.copy() for t in table]
    out[i][b, c, y, x] = v
    return out


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_a_weight_of_zero_skips_its_term(past):
    """Each weight at 0 in turn: the result is the definition's without that term, and a NaN in the skipped term's input does not reach
    the elements that only that term would have spread it to -- which are NaN with the term on."""
    H, W, y, x = 16, 16, 8, 9
    table, ref = TL.tables(H, W, 2, past, tame=True)
    per = 5 if past else 4
    table = [t.copy() for t in table]
    for t in table[:per - 2]:       # the pixel and its neighbours: zero flows (targets inside), plain probabilities
        t[:, :, y - 1:y + 2, x - 1:x + 2] = np.float32(0.5) if t is table[per - 3] else np.float32(0)
    nan = np.float32(np.nan)
    i_o, i_iw1 = per - 3, per - 2
    # (term, the poked tensor / channel, the output tensor / channel / pixel that only this term makes NaN)
    cases = [("smooth_flow", (0, 0), (0, 0, y, x + 1)), ("pme", (i_iw1, 2), (i_o, 1, y, x)), ("smooth_occ", (i_o, 0), (i_o, 0, y + 1, x)),
             ("prior_occ", (i_o, 1), (i_o, 0, y, x))]
    if past:
        cases += [("const_vel", (0, 0), (1, 0, y, x)), ("smooth_flow", (1, 1), (1, 1, y - 1, x))]
    for term, (ti, tc), (gi, gc, gy, gx) in cases:
        bad = poke(table, ti, 0, tc, y, x, nan)
        off = TG.options(**{term: 0.0})
        got_off = check_host(bad, ref, past, 20.0, off)
        got_on = check_host(bad, ref, past, 20.0, TG.DEFAULTS)
        assert np.isnan(got_on[gi][0, gc, gy, gx]), term
        assert np.isfinite(got_off[gi][0, gc, gy, gx]), term
        assert np.isfinite(got_off[gi][1]).all(), term                   # image 1 has no NaN at all
    if not past:        # a Hard table without the smoothness: its flow gradient is +0.0 everywhere
        g = ops.table_loss_grad(table, ref, options=TG.struct(TG.options(smooth_flow=0.0)))
        assert not g[0].view(np.uint32).any()
    g = ops.table_loss_grad(table, ref, options=TG.struct(TG.options(pme=0.0)))
    assert not g[per - 2].view(np.uint32).any() and not g[per - 1].view(np.uint32).any()


# ---- (b) the definition against the reference's updateGradInput functions ----

@pytest.mark.parametrize("variant", ["default", "size_average", "weights"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)])
def test_definition_against_the_lua_gradients(H, W, L, past, variant):
    """Per element |want - lua| <= 2^-24 |v| + 2^-149 + 2^-50 * (the sum of the magnitudes of the element's terms).  Derivation: `want`
    is the fp64 sum rounded to fp32 once -- half an ulp, 2^-24 |v| for a normal v, at most 2^-149 for a subnormal one; before the
    rounding the two sides differ in the exponential alone (loss_exp against np.exp: 2^-50 relative, test_exponential_against_numpy of
    tests/test_table_loss_cpu.py), which scales every smoothness term by (1 + 2^-50) at most, and in fp64 roundings of a few 2^-53 of
    the same terms.  (The transcription also rounds the exponential's argument differently -- -20 * mean against -20 * sum / 3.0 --
    which is |t| 2^-53 relative in the weight, more than 2^-50 for |t| > 8; the printed second figure shows it: before the rounding
    the two sides differ by up to about eight times the bar's fp64 part, in elements where the fp32 part is far larger.)  Nothing is
    tuned."""
    table, ref = tables(H, W, L, past, True)
    o = TG.options(**(OTHER if variant == "weights" else {}))
    o["size_average"] = variant == "size_average"
    per = 5 if past else 4
    for j in range(L):      # the 0-based fp32 mask of the definition and the 1-based one of OBCCriterion.lua:173-176 agree on every pixel
        k = float(np.float32(TL.SCALE / 2.0 ** j))
        for d, fl in enumerate((table[j * per + (1 if past else 0)], table[j * per])):
            zero_based, one_based = TL.inside_masks(fl, -k if d == 0 else k)
            assert (zero_based == one_based).all(), (j, d)
    want, mag, want64 = TG.want_grad(table, ref, past, o=o, with_mag=True)
    lua = TG.lua_grad(table, ref, past, o=o)
    worst = worst64 = 0.0
    for i, (w, m, w64, l) in enumerate(zip(want, mag, want64, lua)):
        assert np.isfinite(w).all() and np.isfinite(l).all()
        bar = 2.0 ** -24 * np.abs(l) + 2.0 ** -149 + 2.0 ** -50 * m
        frac = float((np.abs(w.astype(np.float64) - l) / bar).max())
        worst = max(worst, frac)
        # (for the record: the part of the difference that is there before the rounding, against the exponential's share of the bar)
        worst64 = max(worst64, float((np.abs(w64 - l) / (2.0 ** -50 * m + 2.0 ** -149)).max()))
        assert frac <= 1.0, (i, frac)
    assert sum(float(np.abs(l).max()) > 0 for l in lua) >= len(lua) - 2 * L          # (on a tiny level every target may leave the image)
    print("H %d W %d L %d past %d %s: largest fraction of the bar %.3f; before the rounding, of its fp64 part %.3f" % (H, W, L, past, variant, worst, worst64))


# ---- (c) the reference's gradients against torch.autograd of its forward criteria ----

@pytest.mark.parametrize("size_average", [False, True], ids=["sum", "size_average"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_lua_gradients_against_autograd(past, size_average):
    """Zero difference on f, p, iw1 and iw3; on o the reference is larger by k_pr (quirk 1) plus k_p where the direction's target
    leaves the image (quirk 2).  With size_average the constant-velocity output is given its gradient's norm 1 / (h w) (quirk 3:
    the output's own 1 / (2 h w) halves the derivative)."""
    import torch
    H, W, L = 48, 80, 5
    table, ref = tables(H, W, L, past, True)
    per = 5 if past else 4
    if past:
        table = TG.offset_past(table)
        for j in range(L):
            d = table[5 * j].astype(np.float64) - table[5 * j + 1].astype(np.float64)
            mag = np.sqrt((d * d).sum(axis=1))
            assert mag.min() > 0.04 and mag.max() < 0.51            # every pixel, none left out
    o = TG.options(size_average=size_average)
    lua = TG.lua_grad(table, ref, past, o=o)
    tens = [torch.tensor(t.astype(np.float64), requires_grad=True) for t in table]
    TG.torch_loss(tens, ref, past, o=o, cv_norm_of_gradient=True).backward()
    for j in range(L):
        h, w = H >> j, W >> j
        _, k_cv, k_p, _, k_pr = TG.coefficients(o, j, h, w)
        kd = float(np.float32(TL.SCALE / 2.0 ** j))
        for i in range(per):
            got, auto = lua[j * per + i], tens[j * per + i].grad.numpy()
            expect = np.zeros_like(got)
            if i == per - 3:
                for d in range(2):
                    fl = table[j * per + 1] if (d == 0 and past) else table[j * per]
                    zero_based, one_based = TL.inside_masks(fl, -kd if d == 0 else kd)
                    assert (zero_based == one_based).all()
                    expect[:, 1 - d] = k_pr + k_p * (1.0 - one_based)
                assert j > 0 or ((expect[:, 0] > k_pr).any() and (expect[:, 0] == k_pr).any())        # both kinds of pixel at full size
            # the bar: 64 fp64 roundings of the element's magnitude (each side is a sum of a few products); on the flows of a Soft table
            # also the 1e-12 that ConstVelCriterion.lua:60 adds to the denominator and the derivative has not: k_cv * 1e-12 / |f - p|,
            # |f - p| > 0.04 on every pixel
            atol = 64.0 * 2.0 ** -53 * max(1.0, float(np.abs(got).max())) + (k_cv * 1e-12 / 0.04 if (past and i < 2) else 0.0)
            np.testing.assert_allclose(got - auto, expect, rtol=0, atol=atol, err_msg="level %d tensor %d" % (j, i))
    assert sum(float(np.abs(g).max()) > 0 for g in lua) >= len(lua) - 2


# ---- (d) argument errors, each with nothing written ----

def _call_host(table, ref, grad, past, opts=None, n_outs=None, H=None, W=None):
    n = ref.shape[0]
    tp = (_lib.c_float_p * len(table))(*[_lib.fptr(t) for t in table])
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
    return _lib.lib().b2f_table_loss_grad_host(tp, len(table) if n_outs is None else n_outs, n, H or ref.shape[2], W or ref.shape[3], int(past),
                                               _lib.fptr(ref), 20.0, C.byref(opts) if opts is not None else None, gp)


def test_malformed_requests_are_refused_with_nothing_written():
    table, ref = TL.tables(16, 16, 2, False, tame=True)
    grad = [np.full(t.shape, 7.0, np.float32) for t in table]

    def refused(rc, match):
        with pytest.raises(_lib.B2FError, match=match):
            _lib.check(rc)
        assert all((g == 7.0).all() for g in grad)

    assert _call_host(table, ref, grad, False) == 0 and not any((g == 7.0).all() for g in grad)
    for g in grad:
        g[...] = 7.0
    before = [t.copy() for t in table] + [ref.copy()]
    refused(_call_host(table, ref, [table[0]] + grad[1:], False), "alias")                    # an output is a tensor of the table
    refused(_call_host(table, ref, grad[:3] + [table[6]] + grad[4:], False), "alias")         # ... of another level
    refused(_call_host(table, ref, grad[:7] + [ref], False), "alias")   # ... ref
    refused(_call_host(table, ref, [grad[1]] + grad[1:], False), "alias")                     # two outputs share a buffer
    for t, b in zip(table + [ref], before):
        np.testing.assert_array_equal(t, b)
    for field, value in (("pme", -1.0), ("smooth_occ", float("nan")), ("const_vel", float("inf"))):
        o = back2future.loss_grad_options()
        setattr(o, field, value)
        refused(_call_host(table, ref, grad, False, opts=o), "finite and >= 0")
    o = back2future.loss_grad_options()
    o.level_weights[6] = -0.5
    refused(_call_host(table, ref, grad, False, opts=o), "finite and >= 0")
    refused(_call_host(table, ref, grad, True), "n_outs")                                      # 8 tensors are no Soft table
    refused(_call_host(table[:7], ref, grad[:7], False), "n_outs")
    big = [np.zeros((1, 3 if i % 4 >= 2 else 2, 128 >> (i // 4), 128 >> (i // 4)), np.float32) for i in range(32)]
    out = [np.full(t.shape, 7.0, np.float32) for t in big]
    with pytest.raises(_lib.B2FError, match="1 .. 7 levels"):
        _lib.check(_call_host(big, np.zeros((1, 3, 128, 128), np.float32), out, False))
    assert all((g == 7.0).all() for g in out)
    with pytest.raises(ValueError, match="finite and >= 0"):
        back2future.loss_grad_options(weights={"pme": -2.0})
    with pytest.raises(ValueError, match="unknown weight"):
        back2future.loss_grad_options(weights={"entropy": 1.0})


def test_which_refusal_is_reported_when_two_apply():
    """The order of an entry's checks is part of what a caller sees.  The host entry looks at the table before the options; the device
    entry looks at its options before its context, while the entries of the records and of the supervised objective look at the context
    first (a null context: no GPU is touched)."""
    table, ref = TL.tables(16, 16, 2, False, tame=True)
    grad = [np.full(t.shape, 7.0, np.float32) for t in table]
    bad = back2future.loss_grad_options()
    bad.pme = -1.0
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_grad_host: n_outs"):
        _lib.check(_call_host(table[:7], ref, grad[:7], False, opts=bad))
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_grad_host: the gradient table must not alias"):
        _lib.check(_call_host(table, ref, [table[0]] + grad[1:], False, opts=bad))
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_grad_host: .*finite and >= 0"):
        _lib.check(_call_host(table, ref, grad, False, opts=bad))
    lib = _lib.lib()
    tp = (C.c_void_p * len(table))(*[t.ctypes.data for t in table])
    gp = (C.c_void_p * len(grad))(*[g.ctypes.data for g in grad])
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_grad_device: .*finite and >= 0"):
        _lib.check(lib.b2f_table_loss_grad_device(None, tp, len(table), 2, 16, 16, ref.ctypes.data, 20.0, C.byref(bad), gp, None))
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_grad_device: null context"):
        _lib.check(lib.b2f_table_loss_grad_device(None, tp, 7, 2, 16, 16, ref.ctypes.data, 20.0, None, gp, None))
    loss = np.full((2, 2, back2future.LOSS_SSIM_WORDS), 7, np.uint64)
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_ssim_device: null context"):      # a range_mode that does not exist
        _lib.check(lib.b2f_table_loss_ssim_device(None, tp, len(table), 2, 16, 16, ref.ctypes.data, 20.0, loss.ctypes.data, None, 9, None))
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: null context"):       # a count_mode that does not exist
        _lib.check(lib.b2f_table_loss_epe_device(None, tp, len(table), 2, 16, 16, ref.ctypes.data, None, None, 20.0, None, 9, None, loss.ctypes.data, gp, None))
    assert all((g == 7.0).all() for g in grad) and (loss == 7).all()


@pytest.mark.parametrize("name", ["Ours-Soft-ft-KITTI", "Ours-Soft-ft-Sintel"])
def test_the_fine_tuning_objectives_are_refused(name):
    with pytest.raises(ValueError, match="gradient of objective %r is not provided.*SecondOrderSmoothnessCriterion.*OBGCCriterion" % name):
        back2future.loss_grad_options(objective=name)
    with pytest.raises(ValueError, match="unknown objective"):
        back2future.loss_grad_options(objective="Ours-Medium")
