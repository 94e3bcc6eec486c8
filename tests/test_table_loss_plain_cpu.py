"""CPU: the photometric terms without occlusion masking (include/b2f.h, the *_plain and *_grad_plain entries; criterions/MBCCriterion.lua,
criterions/MSSIML1Criterion.lua; -no_occ) without a GPU: (a) the host entries equal the numpy restatement of the definition with no
tolerance, every record word and every gradient element, words 0 .. 15 those of b2f_table_loss_host; (b) the restatement agrees with a
float64 transcription of the Lua within derived bounds; (c) identities against the entries that exist: with occlusions of 1 the sums
are those of the occlusion-aware records and the image planes those of the occlusion-aware gradients, bit for bit, and with pme = 0
every element is b2f_table_loss_grad_ft_host's; (d) the transcription equals torch.autograd where the Lua is a derivative, a target
outside the image gives exactly nothing, and the range reaches over the occlusions and the past flow; (e) wrong readings are told from
the definition; (f) malformed requests are refused with nothing written; (g) the symbols, the struct, the defaults, the version."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL
from tests import table_loss_grad_ft_fields as TF
from tests import table_loss_grad_ssim as TGS
from tests import table_loss_plain_fields as TP
from tests import table_loss_ssim_fields as TS
from tests import test_table_loss_grad_ssim_cpu as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_table_loss_plain_host", "b2f_table_loss_plain_device", "b2f_op_table_loss_plain", "b2f_forward_loss_plain", "b2f_forward_loss_plain_device",
           "b2f_multi_forward_loss_plain"]
GRAD_ENTRIES = ["b2f_loss_grad_plain_defaults", "b2f_table_loss_grad_plain_host", "b2f_table_loss_grad_plain_device", "b2f_op_table_loss_grad_plain",
                "b2f_forward_loss_grad_plain", "b2f_forward_loss_grad_plain_device", "b2f_multi_forward_loss_grad_plain"]
# 1 x 1 .. 5 x 7: every border case of the 3 x 3 window and of the five-point cross; 37 x 53: odd, several groups per row;
# (16,16,5): the coarsest levels are 2 x 2 and 1 x 1; (48,80,5): widths 80 .. 5
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
F32 = np.float32
# BCC with both penalties; SSIM with alpha 1 / 0.85 / 0.5 / 0
CRITERIA = [dict(pme_criterion="BCC"), dict(pme_criterion="BCC", pme_penalty="Quadratic"), dict(pme_criterion="SSIM"), dict(pme_criterion="SSIML1"),
            dict(pme_criterion="SSIM", ssim_alpha=0.5), dict(pme_criterion="SSIM", ssim_alpha=0.0)]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


_TABLES = {}


def tables(H, W, L, past, tame):
    """the tables of table_loss_fields, computed once and left unchanged"""
    key = (H, W, L, past, tame)
    if key not in _TABLES:
        _TABLES[key] = TL.tables(H, W, L, past, tame=tame)
    return _TABLES[key]


same_bits = GS.same_bits


def given(L):
    """a range per level that holds the tame fields' values without being anyone's own"""
    return np.array([[-3.0 - 0.25 * j, 3.5 + 0.125 * j] for j in range(L)], F32)


def records(table, ref, flow_scale, mode, ranges):
    return ops.table_loss(table, ref, flow_scale=flow_scale, objective="plain", ssim_range=TP.range_arg(mode, ranges))


def grads(table, ref, flow_scale, o, mode, ranges):
    return ops.table_loss_grad(table, ref, flow_scale=flow_scale, options=TP.struct(o), ssim_range=TP.range_arg(mode, ranges))


def check_grad(table, ref, past, flow_scale, o, mode=TP.BATCH, ranges=None, what=""):
    got = grads(table, ref, flow_scale, o, mode, ranges)
    want = TP.want_grad_plain(table, ref, past, flow_scale, o, mode, ranges)
    assert len(got) == len(want) == len(table)
    for i, (g, w) in enumerate(zip(got, want)):
        same_bits(g, w, "%s tensor %d" % (what, i))
    return got


# ---- (g) symbols, struct, defaults, version ----

def test_symbols_struct_defaults_and_version():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES + GRAD_ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in doc and name + "(" in cdef, name
    for name in ENTRIES:                                       # the argument list of the _ssim sibling
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_plain", "_ssim")], name
    for name in GRAD_ENTRIES[1:]:                              # ... with the options' own pointer type
        a, b = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name.replace("_plain", "_ssim")][1]
        assert [_lib.c_grad_ssim_opts_p if t is _lib.c_grad_plain_opts_p else t for t in a] == b, name
    assert _lib.lib().b2f_version() >= 1013
    words = dict((k, int(v)) for k, v in re.findall(r"#define (B2F_LOSS_PLAIN_\w+) (\d+)", hdr))
    assert words == {"B2F_LOSS_PLAIN_L1_Q30": 16, "B2F_LOSS_PLAIN_SQ_Q30": 18, "B2F_LOSS_PLAIN_SSIM_Q30": 20, "B2F_LOSS_PLAIN_L1N_Q30": 22,
                     "B2F_LOSS_PLAIN_SSIM_NONFINITE": 24, "B2F_LOSS_PLAIN_RANGE_USED": 26, "B2F_LOSS_PLAIN_RANGE_OWN": 28, "B2F_LOSS_PLAIN_WORDS": 40}
    for k, v in words.items():
        assert getattr(back2future, k[4:]) == v, k
    assert (TP.WORDS, TP.L1, TP.SQ, TP.SSIM, TP.L1N, TP.SSIM_NONFINITE, TP.RANGE_USED, TP.RANGE_OWN) == (40, 16, 18, 20, 22, 24, 26, 28)
    kinds = dict((k, int(v)) for k, v in re.findall(r"#define (B2F_PLAIN_\w+) (\d+)", hdr))
    assert kinds == {"B2F_PLAIN_BCC": 0, "B2F_PLAIN_SSIM": 1, "B2F_PLAIN_L1": 0, "B2F_PLAIN_QUADRATIC": 1}
    assert (back2future.PLAIN_BCC, back2future.PLAIN_SSIM, back2future.PLAIN_L1, back2future.PLAIN_QUADRATIC) == (0, 1, 0, 1)
    assert [back2future.loss_words(k) for k in ("pme", "finetune", "ssim", "plain", "epe")] == [16, 24, 32, 40, 8]
    assert back2future.PLAIN_ALPHA == TP.ALPHA == {"SSIM": 1.0, "SSIML1": 0.85}
    # the structs: the older ones unchanged; the new one 12 doubles, four ints, alpha
    assert C.sizeof(_lib.LossGradOpts) == 104 and C.sizeof(_lib.LossGradFtOpts) == 136 and C.sizeof(_lib.LossGradSsimOpts) == 12 * 8 + 2 * 4 + 8
    assert C.sizeof(_lib.LossGradPlainOpts) == 12 * 8 + 4 * 4 + 8
    o = back2future.loss_grad_plain_options()
    d = back2future.loss_grad_options()
    assert [getattr(o, k) for k in TP.TERMS] == [getattr(d, k) for k in TP.TERMS]
    assert tuple(o.level_weights) == back2future.LOSS_LEVEL_WEIGHTS and o.size_average == 0
    assert (o.smooth_second_order, o.criterion, o.penalty, o.ssim_alpha) == (0, 0, 0, 0.85)
    s = back2future.loss_grad_plain_options(pme_criterion="SSIM", smooth_second_order=True, size_average=True, weights={"pme": 3.0}, no_occ=True)
    assert (s.criterion, s.ssim_alpha, s.smooth_second_order, s.size_average, s.pme, s.smooth_occ, s.prior_occ) == (1, 1.0, 1, 1, 3.0, 0.0, 0.0)
    assert back2future.loss_grad_plain_options(pme_criterion="SSIML1").ssim_alpha == 0.85
    assert back2future.loss_grad_plain_options(pme_criterion="SSIM", ssim_alpha=0.25).ssim_alpha == 0.25
    assert back2future.loss_grad_plain_options(pme_penalty="Quadratic").penalty == 1
    for kw in (dict(pme_criterion="SSIM", ssim_alpha=-0.1), dict(pme_criterion="SSIM", ssim_alpha=float("nan")), dict(pme_criterion="OBCC"),
               dict(pme_criterion="SSIM", pme_penalty="Quadratic"), dict(pme_penalty="Lorentzian"), dict(ssim_alpha=0.5)):
        with pytest.raises(ValueError):
            back2future.loss_grad_plain_options(**kw)
    for src, cite in (("b2f_tableloss_plain.h", "MBCCriterion.lua:35-186"), ("b2f_tableloss_plain.hip", "MSSIML1Criterion.lua:45-153"),
                      ("b2f_tableloss_grad_plain.hip", "MSSIML1Criterion.lua:155-261")):
        assert cite in open(os.path.join(ROOT, "back2future_amd", "csrc", src)).read(), src


# ---- (a) the host entries against the definition, with no tolerance ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_records_equal_the_existing_records_and_the_definition(H, W, L, past):
    """wild and tame tables x flow_scale 20 and 10 x the three range modes and a given range that does not hold the values"""
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        for scale in (20.0, 10.0):
            base = ops.table_loss(table, ref, flow_scale=scale)
            for mode, ranges in ((TP.BATCH, None), (TP.IMAGE, None), (TP.GIVEN, given(L)), (TP.GIVEN, GS.wide_ranges(L))):
                got = records(table, ref, scale, mode, ranges)
                want = TP.want_plain(table, ref, past, scale, mode, ranges)
                assert got.shape == (2, L, 40) and got.dtype == np.uint64
                np.testing.assert_array_equal(got[:, :, :16], base)
                for word in range(16, 30):
                    np.testing.assert_array_equal(got[:, :, word], want[:, :, word - 16], err_msg="word %d tame %d scale %g mode %d" % (word, tame, scale, mode))
                assert not got[:, :, 30:].any()
                if mode == TP.GIVEN:
                    assert (got[:, :, TP.RANGE_USED:TP.RANGE_USED + 2].astype(np.uint32).view(F32) == ranges[None]).all()


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_gradient_equals_the_definition(H, W, L, past):
    """wild and tame tables x the criteria x the range modes x second order x size_average x flow_scale 10, then each weight at 0 and no_occ"""
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        for i, c in enumerate(CRITERIA):
            second, avg = bool(i & 1), bool(i & 2)
            o = TP.options(smooth_second_order=second, size_average=avg, **c)
            for mode, ranges in ((TP.BATCH, None), (TP.IMAGE, None), (TP.GIVEN, given(L)), (TP.GIVEN, GS.wide_ranges(L))):
                if c["pme_criterion"] == "BCC" and mode != TP.BATCH:       # BCC does not read the range
                    continue
                check_grad(table, ref, past, 20.0, o, mode, ranges, "tame %d %r mode %d" % (tame, c, mode))
            check_grad(table, ref, past, 10.0, o, TP.BATCH, None, "tame %d %r scale 10" % (tame, c))
        for c in (CRITERIA[0], CRITERIA[3]):
            for k in TP.TERMS:
                check_grad(table, ref, past, 20.0, TP.options(**dict(c, **{k: 0.0})), TP.IMAGE, None, "%s = 0 tame %d" % (k, tame))
            got = check_grad(table, ref, past, 20.0, TP.options(no_occ=True, **c), TP.IMAGE, None, "no_occ tame %d" % tame)
            per = 5 if past else 4
            for j in range(L):      # -no_occ: the occlusion planes are +0.0
                assert not got[j * per + per - 3].view(np.uint32).any()


# ---- (c) identities against the entries that exist ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (37, 53, 1), (48, 80, 5)])
def test_with_occlusions_of_one_it_is_the_occlusion_aware_code(H, W, L, past):
    per = 5 if past else 4
    for tame in (False, True):
        table, ref = tables(H, W, L, past, tame)
        table = [np.ones_like(t) if i % per == per - 3 else t for i, t in enumerate(table)]
        rng = given(L)       # the same range given to both: the plain entries' own range reaches over the occlusions
        got = records(table, ref, 20.0, TP.GIVEN, rng)
        ssim = ops.table_loss(table, ref, objective="ssim", ssim_range=rng)
        np.testing.assert_array_equal(got[:, :, TP.L1:TP.L1 + 2], got[:, :, back2future.LOSS_PHOTO_OCHARB_Q30:back2future.LOSS_PHOTO_OCHARB_Q30 + 2])
        np.testing.assert_array_equal(got[:, :, TP.SSIM:TP.SSIM + 2], ssim[:, :, TS.SSIM:TS.SSIM + 2])
        np.testing.assert_array_equal(got[:, :, TP.L1N:TP.L1N + 2], ssim[:, :, TS.L1N:TS.L1N + 2])
        np.testing.assert_array_equal(got[:, :, TP.SSIM_NONFINITE:TP.SSIM_NONFINITE + 2], ssim[:, :, TS.SSIM_NONFINITE:TS.SSIM_NONFINITE + 2])
        for second in (False, True):
            o = TP.options(smooth_occ=0.0, prior_occ=0.0, smooth_second_order=second)
            a = grads(table, ref, 20.0, o, TP.BATCH, None)
            b = ops.table_loss_grad(table, ref, options=TF.struct(TGS.ft_options(o)))
            for j in range(L):
                for i in (per - 2, per - 1):
                    same_bits(a[j * per + i], b[j * per + i], "BCC / L1 image plane %d of level %d" % (i, j))
            for alpha in (1.0, 0.85, 0.0):
                o = TP.options(pme_criterion="SSIM", ssim_alpha=alpha, smooth_occ=0.0, prior_occ=0.0, smooth_second_order=second)
                a = grads(table, ref, 20.0, o, TP.GIVEN, rng)
                b = ops.table_loss_grad(table, ref, options=TGS.struct(TGS.options(ssim_alpha=alpha, smooth_occ=0.0, prior_occ=0.0, smooth_second_order=second)),
                                        ssim_range=rng)
                for j in range(L):
                    for i in (per - 2, per - 1):
                        same_bits(a[j * per + i], b[j * per + i], "SSIM alpha %g image plane %d of level %d" % (alpha, i, j))


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_without_pme_it_is_the_fine_tuning_entry(past):
    table, ref = tables(48, 80, 5, past, False)
    for c in (CRITERIA[0], CRITERIA[1], CRITERIA[3]):
        for second in (False, True):
            o = TP.options(pme=0.0, smooth_second_order=second, **c)
            a = grads(table, ref, 20.0, o, TP.IMAGE, None)
            b = ops.table_loss_grad(table, ref, options=TF.struct(TGS.ft_options(o)))
            for i, (g, w) in enumerate(zip(a, b)):
                same_bits(g, w, "pme 0 %r tensor %d" % (c, i))


# ---- (b) the restatement against the transcription of the Lua ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("criterion,penalty", [("BCC", "L1"), ("BCC", "Quadratic"), ("SSIM", "L1"), ("SSIML1", "L1")])
def test_loss_summary_agrees_with_the_lua(criterion, penalty, past):
    """loss_summary over the host records against the float64 transcription per triplet, like test and train, with and without
    size_average and no_occ; tame tables (no saturated term), the range of the triplet alone (batch=False) in image mode and of the
    batch in batch mode.  The bar is bound_plain's (derived there); the largest share used is printed.  With the quadratic penalty the
    images are taken at a quarter of their values (exact in fp32): the sum of three squared differences of the tame fields reaches 70,
    and q saturates at 16, which the Lua does not."""
    worst = 0.0
    per = 5 if past else 4
    for (H, W, L) in ((5, 7, 1), (37, 53, 1), (48, 80, 5)):
        table, ref = tables(H, W, L, past, True)
        if penalty == "Quadratic":
            table, ref = [t * F32(0.25) if i % per >= per - 2 else t for i, t in enumerate(table)], ref * F32(0.25)
        for like, avg, no_occ, batch in (("test", False, False, True), ("train", True, True, False), ("train", False, True, True)):
            rec = records(table, ref, 20.0, TP.BATCH if batch else TP.IMAGE, None)
            s = back2future.loss_summary(rec, like=like, size_average=avg, pme_criterion=criterion, pme_penalty=penalty, no_occ=no_occ)
            lua = TP.lua_loss_plain(table, ref, past, criterion, penalty, like=like, size_average=avg, batch=batch, no_occ=no_occ)
            assert s["nonfinite"] == 0
            for b in range(2):
                bar = TP.bound_plain(H, W, L, past, criterion, like=like, size_average=avg, lua=lua[b], no_occ=no_occ)
                err = abs(float(s["loss"][b]) - lua[b])
                worst = max(worst, err / bar)
                assert err <= bar, "%dx%d %s avg %d no_occ %d: %r against %r, bar %g" % (H, W, like, avg, no_occ, float(s["loss"][b]), lua[b], bar)
            # -no_occ drops exactly the two occlusion terms
            full = back2future.loss_summary(rec, like=like, size_average=avg, pme_criterion=criterion, pme_penalty=penalty)
            lw = np.asarray(back2future.LOSS_LEVEL_WEIGHTS[:L])[None]
            drop = (lw * (0.1 * full["smooth_occ"] + 0.1 * full["prior_occ"])).sum(axis=1)
            np.testing.assert_allclose(full["loss"] - drop, back2future.loss_summary(rec, like=like, size_average=avg, pme_criterion=criterion,
                                                                                      pme_penalty=penalty, no_occ=True)["loss"], rtol=1e-13)
    print("largest share of the bar used: %.3g" % worst)


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("c", [0, 1, 2, 3, 5])
def test_gradient_restatement_agrees_with_the_lua(past, c):
    """per element within 2^-24 |v| + 2^-149 + a m: a = allowance_bcc_grad() for BCC (counted there), allowance_ssim_grad() of the
    existing helper for SSIM (derived there with the factor o <= 1 counted as 1: it applies unchanged without it); m the sum of the
    magnitudes of the element's terms; tame tables, the batch range, which holds the values"""
    crit = CRITERIA[c]
    a = TP.allowance_bcc_grad() if crit["pme_criterion"] == "BCC" else TGS.allowance_ssim_grad()
    worst = 0.0
    for (H, W, L) in ((5, 7, 1), (37, 53, 1), (48, 80, 5)):
        table, ref = tables(H, W, L, past, True)
        for second, avg, no_occ in ((False, False, False), (True, True, True)):
            o = TP.options(smooth_second_order=second, size_average=avg, no_occ=no_occ, **crit)
            want, mags, sums = TP.want_grad_plain(table, ref, past, 20.0, o, TP.BATCH, None, with_mag=True)
            lua = TP.lua_grad_plain(table, ref, past, 20.0, o)
            per = 5 if past else 4
            rest = TF.want_grad_ft(table, ref, past, 20.0, TGS.ft_options(o, pme=0.0))
            for i, (w, l, m, s64) in enumerate(zip(want, lua, mags, sums)):
                if m is None:       # the flow planes: tests/test_table_loss_grad_ft_cpu.py holds them
                    continue
                if i % per == per - 3:
                    # the occlusion planes read no photometric term: they are those of the fine-tuning definition without pme, bit for
                    # bit, which tests/test_table_loss_grad_ft_cpu.py holds to the Lua with the bar of the contrast weights
                    same_bits(w, rest[i], "occlusion plane %d" % i)
                    if crit["pme_criterion"] == "BCC":
                        continue
                bar = 2.0 ** -24 * np.abs(l) + 2.0 ** -149 + a * m
                err = np.abs(w.astype(np.float64) - l)
                share = float((np.abs(s64 - l) / (a * m + 1e-300)).max())
                worst = max(worst, share)
                assert share <= 1.0 and (err <= bar).all(), "tensor %d of %d x %d: share of the fp64 part %g" % (i, H, W, share)
    print("largest share of a m used: %.3g" % worst)


# ---- (d) behaviour ----

@pytest.mark.parametrize("penalty", ["L1", "Quadratic"])
def test_bcc_gradient_is_the_autograd_of_its_value(penalty):
    """48 x 80: MBCCriterion:updateGradInput equals torch.autograd of updateOutput within 64 fp64 roundings of the element's magnitude
    (the mask does not depend on the images)"""
    import torch
    table, ref = tables(48, 80, 1, True, True)
    sub = [t[:1] for t in table]
    xs = [torch.from_numpy(sub[3].astype(np.float64)).requires_grad_(True), torch.from_numpy(sub[4].astype(np.float64)).requires_grad_(True)]
    for avg in (False, True):
        v = TP.mbcc(sub, ref[:1], True, 20.0, penalty, avg, tensors=xs)
        g = torch.autograd.grad(v, xs)
        back = TP.mbcc_back(sub, ref[:1], True, 20.0, penalty, avg)
        assert not back[0].any()                                                       # gradInput[1]:fill(0)
        for d in range(2):
            err = np.abs(back[1 + d] - g[d].numpy())
            assert (err <= 64 * 2.0 ** -53 * np.abs(back[1 + d]) + 1e-300).all()
            assert np.abs(back[1 + d]).max() > 0


@pytest.mark.parametrize("alpha", [1.0, 0.85])
def test_ssim_gradient_is_the_own_window_diagonal_inside_and_not_on_the_border(alpha):
    """zero flows (every target inside), 48 x 80, given range (0, 1): at interior pixels MSSIML1Criterion:updateGradInput's image gradient
    equals the autograd of the pixel's own window term within 64 fp64 roundings of the terms' magnitudes (the eight neighbouring
    windows are dropped); on the border it does not (gw = gc^2 there too); with range (0, 2) the two differ by the missing 1 / (mx - mn)"""
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
        back = TP.mssiml1_back(sub, target, False, 20.0, alpha, mn, mx, False)
        assert not back[0].any()                                                       # gradInput[1]:fill(0)
        for d in range(2):
            y = torch.from_numpy(target.astype(np.float64))
            x = torch.from_numpy(sub[2 + d].astype(np.float64)).requires_grad_(True)
            terms, scale = GS._own_window_terms(x, y, torch.ones(1, 1, H, W, dtype=torch.float64), alpha, (mn, mx))
            diag = np.zeros((1, 3, H, W))
            for oy in range(3):
                for ox in range(3):
                    (g,) = torch.autograd.grad(terms[:, :, oy::3, ox::3].sum(), x, retain_graph=True)
                    diag[:, :, oy::3, ox::3] = g.numpy()[:, :, oy::3, ox::3]
            lua = back[1 + d] * 6.0 / (mx - mn)
            err = np.abs(lua - diag)
            share = (err[:, :, interior] / (64 * 2.0 ** -53 * scale[:, :, interior] + 1e-300)).max()
            print("alpha %g range (%g, %g) direction %d: share of 64 roundings used %.3g" % (alpha, mn, mx, d, share))
            assert share <= 1.0
            assert (err[:, :, ~interior] > 1e-6).any()
            if mx - mn != 1.0:
                assert np.abs(back[1 + d] * 6.0 - diag)[:, :, interior].max() > 1e-6


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_a_target_outside_the_image_gives_exactly_nothing(past):
    """flows that send every target of one direction off the image: that direction's words are 0 and its image planes +0.0, in every
    criterion; the other direction is untouched"""
    per = 5 if past else 4
    table, ref = tables(5, 7, 1, past, True)
    base = records(table, ref, 20.0, TP.IMAGE, None)
    out = [t.copy() for t in table]
    out[0][:] = 1.0                        # the future flow: 20 pixels to the right and down, off a 5 x 7 image
    rec = records(out, ref, 20.0, TP.IMAGE, None)
    d_out = (1,) if past else (0, 1)       # on a Hard table the future flow also moves the past frame's target (by -20)
    for d in d_out:
        assert not rec[:, :, [TP.L1 + d, TP.SQ + d, TP.SSIM + d, TP.L1N + d, TP.SSIM_NONFINITE + d]].any()
        assert (rec[:, :, back2future.LOSS_PHOTO_OUTSIDE + d] == 35).all()
    if past:
        np.testing.assert_array_equal(rec[:, :, [TP.L1, TP.SQ, TP.SSIM, TP.L1N]], base[:, :, [TP.L1, TP.SQ, TP.SSIM, TP.L1N]])
    s = back2future.loss_summary(rec, pme_criterion="BCC")
    if not past:
        assert not s["pme"].any()          # no penalty_out: nothing inside, nothing added
    for c in CRITERIA:
        g = grads(out, ref, 20.0, TP.options(**c), TP.IMAGE, None)
        for d in d_out:
            assert not g[per - 2 + d].view(np.uint32).any(), c
        if past:
            assert g[per - 2].any()


def test_the_range_reaches_over_the_occlusions_and_the_past_flow():
    """the quirk of MSSIML1Criterion.lua:63-68: a maximum in an occlusion plane and, on a Soft table, a minimum in the past flow move
    RANGE_OWN and the SSIM words; BCC's words and the first 16 do not move with the past flow's far corner pixel ... the occlusion-aware
    records' range stays where it was"""
    table, ref = tables(5, 7, 1, True, True)
    base = records(table, ref, 20.0, TP.IMAGE, None)
    poked = [t.copy() for t in table]
    poked[2][0, 0, 4, 6] = 9.0             # an occlusion plane holds the maximum
    a = records(poked, ref, 20.0, TP.IMAGE, None)
    own = a[:, :, TP.RANGE_OWN:TP.RANGE_OWN + 2].astype(np.uint32).view(F32)
    assert own[0, 0, 1] == 9.0 and own[1, 0, 1] < 9.0
    assert (a[0, 0, TP.SSIM:TP.SSIM + 2] != base[0, 0, TP.SSIM:TP.SSIM + 2]).all() and (a[0, 0, TP.L1N:TP.L1N + 2] != base[0, 0, TP.L1N:TP.L1N + 2]).all()
    np.testing.assert_array_equal(a[1], base[1])
    poked[1][0, 1, 0, 0] = -11.0           # the past flow holds the minimum (the target of pixel (0, 0) leaves the image with it)
    b = records(poked, ref, 20.0, TP.IMAGE, None)
    own = b[:, :, TP.RANGE_OWN:TP.RANGE_OWN + 2].astype(np.uint32).view(F32)
    assert own[0, 0, 0] == -11.0 and own[0, 0, 1] == 9.0
    assert (b[0, 0, TP.SSIM:TP.SSIM + 2] != a[0, 0, TP.SSIM:TP.SSIM + 2]).all()
    # the occlusion-aware records take their range over the images alone
    s0 = ops.table_loss(table, ref, objective="ssim", ssim_range="image")
    s1 = ops.table_loss(poked, ref, objective="ssim", ssim_range="image")
    np.testing.assert_array_equal(s0[:, :, TS.RANGE_OWN:TS.RANGE_OWN + 2], s1[:, :, TS.RANGE_OWN:TS.RANGE_OWN + 2])
    # the gradient follows the same range
    g0 = grads(table, ref, 20.0, TP.options(pme_criterion="SSIML1"), TP.IMAGE, None)
    g1 = grads(poked, ref, 20.0, TP.options(pme_criterion="SSIML1"), TP.IMAGE, None)
    assert not np.array_equal(g0[4][0], g1[4][0]) and np.array_equal(g0[4][1], g1[4][1])
    # on a Hard table the flow is input[1]: not part of the range
    table, ref = tables(5, 7, 1, False, True)
    poked = [t.copy() for t in table]
    poked[0][0, 1, 0, 0] = -11.0
    np.testing.assert_array_equal(records(poked, ref, 20.0, TP.IMAGE, None)[:, :, TP.RANGE_OWN:TP.RANGE_OWN + 2],
                                  records(table, ref, 20.0, TP.IMAGE, None)[:, :, TP.RANGE_OWN:TP.RANGE_OWN + 2])


def test_a_switched_off_term_is_not_evaluated():
    """pme = 0, or alpha = 0 for the SSIM part: a NaN that only that term reads stays out of the table"""
    table, ref = tables(5, 7, 1, True, True)
    poked = [t.copy() for t in table]
    poked[3][0, 1, 2, 3] = np.nan
    for c in CRITERIA:
        off = grads(poked, ref, 20.0, TP.options(pme=0.0, **c), TP.BATCH, None)
        assert all(np.isfinite(g).all() for g in off) and not off[3].any() and not off[4].any()
    on = grads(poked, ref, 20.0, TP.options(pme_criterion="SSIML1"), TP.GIVEN, given(1))
    assert np.isnan(on[3][0, 1]).any() and np.isfinite(on[3][0, 0]).all() and np.isfinite(on[4]).all() and np.isfinite(on[3][1]).all()
    assert np.isfinite(on[2]).all()        # the occlusions do not read the photometric term


# ---- (e) wrong readings of the definition ----

@pytest.mark.parametrize("mutation", TP.MUTATIONS)
def test_a_wrong_reading_is_told_from_the_definition(mutation):
    """each mutation of the restatement differs from the host entry on the 1 x 5 or the 3 x 3 case, in a record word or a gradient
    element.  The tame fields of these sizes have zero flows and occlusions inside the images' range, so one future flow is set to
    leave the image and one occlusion to 5, above every image value."""
    told = False
    for H, W in ((1, 5), (3, 3)):
        table, ref = tables(H, W, 1, True, True)
        table = [t.copy() for t in table]
        table[0][:, 0, 0, 0] = 3.0
        table[2][:, 1, H - 1, W - 1] = 5.0
        got = records(table, ref, 20.0, TP.BATCH, None)[:, :, 16:30]
        told = told or not np.array_equal(got, TP.want_plain(table, ref, True, 20.0, TP.BATCH, None, mutation=mutation))
        for c in (CRITERIA[1], CRITERIA[3]):
            o = TP.options(**c)
            g = grads(table, ref, 20.0, o, TP.BATCH, None)
            wrong = TP.want_grad_plain(table, ref, True, 20.0, o, TP.BATCH, None, mutation=mutation)
            told = told or any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(g, wrong))
    assert told, mutation


# ---- (f) refusals: nothing is written ----

def test_refusals_write_nothing():
    table, ref = tables(16, 16, 5, True, True)
    n, H, W = ref.shape[0], 16, 16
    lib = _lib.lib()
    grad = [np.full(t.shape, 7.0, np.float32) for t in table]
    loss = np.full((n, 5, 40), 7, np.uint64)
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong))
    ptrs = (_lib.c_float_p * len(table))(*[_lib.fptr(t) for t in table])
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])

    def call(opts=None, n_outs=len(table), g=gp, mode=TP.IMAGE, ranges=None, tab=ptrs, scale=20.0):
        return lib.b2f_table_loss_grad_plain_host(tab, n_outs, n, H, W, 1, _lib.fptr(ref), scale, C.byref(opts) if opts is not None else None, g, mode, ranges)

    def value(n_outs=len(table), mode=TP.IMAGE, ranges=None, out=lp, scale=20.0, r=ref):
        return lib.b2f_table_loss_plain_host(ptrs, n_outs, n, H, W, 1, _lib.fptr(r) if r is not None else None, scale, out, mode, ranges)

    def refused(rc, what):
        assert rc != 0, what
        assert all((x == 7.0).all() for x in grad) and (loss == 7).all(), what + ": written"

    assert call() == 0 and not any((x == 7.0).all() for x in grad)
    assert value() == 0 and not (loss == 7).all()
    for x in grad:
        x.fill(7.0)
    loss.fill(7)
    aliased = (_lib.c_float_p * len(grad))(*([_lib.fptr(table[0])] + [_lib.fptr(g) for g in grad[1:]]))
    refused(call(g=aliased), "aliases the table")
    twice = (_lib.c_float_p * len(grad))(*([_lib.fptr(grad[1])] + [_lib.fptr(g) for g in grad[1:]]))
    refused(call(g=twice), "aliases itself")
    for field, bad in (("pme", -1.0), ("smooth_occ", float("inf")), ("prior_occ", float("nan")), ("ssim_alpha", -0.01), ("ssim_alpha", 1.01),
                       ("ssim_alpha", float("nan")), ("criterion", 2), ("criterion", -1), ("penalty", 2), ("penalty", -1)):
        o = back2future.loss_grad_plain_options()
        setattr(o, field, bad)
        refused(call(opts=o), "%s = %r" % (field, bad))
    o = back2future.loss_grad_plain_options(pme_criterion="SSIM")
    o.penalty = back2future.PLAIN_QUADRATIC
    refused(call(opts=o), "the quadratic penalty with SSIM")
    o = back2future.loss_grad_plain_options()
    o.level_weights[2] = -0.5
    refused(call(opts=o), "level weight")
    for f in (call, value):
        refused(f(mode=3), "range_mode 3")
        refused(f(mode=-1), "range_mode -1")
        refused(f(mode=TP.GIVEN, ranges=None), "given without ranges")
        refused(f(n_outs=len(table) - 1), "n_outs")
        refused(f(n_outs=0), "n_outs 0")
        refused(f(scale=0.0), "flow_scale 0")
        refused(f(scale=float("nan")), "flow_scale NaN")
    refused(value(out=None), "null loss")
    refused(value(r=None), "null ref")
    refused(call(g=None), "null grad")
    # L > 7: eight levels of a Hard table
    big = [np.zeros((1, 2 if i % 4 < 2 else 3, 128 >> (i // 4), 128 >> (i // 4)), np.float32) for i in range(32)]
    bg = [np.full(t.shape, 7.0, np.float32) for t in big]
    bl = np.full((1, 8, 40), 7, np.uint64)
    bp = (_lib.c_float_p * 32)(*[_lib.fptr(t) for t in big])
    zero = np.zeros((1, 3, 128, 128), np.float32)
    assert lib.b2f_table_loss_grad_plain_host(bp, 32, 1, 128, 128, 0, _lib.fptr(zero), 20.0, None, (_lib.c_float_p * 32)(*[_lib.fptr(g) for g in bg]),
                                              TP.IMAGE, None) != 0
    assert lib.b2f_table_loss_plain_host(bp, 32, 1, 128, 128, 0, _lib.fptr(zero), 20.0, bl.ctypes.data_as(C.POINTER(C.c_ulonglong)), TP.IMAGE, None) != 0
    assert all((x == 7.0).all() for x in bg) and (bl == 7).all()
    assert lib.b2f_loss_grad_plain_defaults(None) != 0
    for kw in (dict(ssim_range="neither"), dict(ssim_range=np.zeros((4, 2), np.float32))):
        with pytest.raises(ValueError):
            ops.table_loss_grad(table, ref, options=back2future.loss_grad_plain_options(), **kw)
        with pytest.raises(ValueError):
            ops.table_loss(table, ref, objective="plain", **kw)
    rec = records(table, ref, 20.0, TP.IMAGE, None)
    for kw in (dict(pme_criterion="BCC", pme_penalty="Lorentzian"), dict(pme_criterion="SSIM", pme_penalty="Quadratic"), dict(pme_criterion="MBCC"),
               dict(pme_criterion="BCC", ssim_alpha=0.5), dict(pme_criterion="SSIM", ssim_alpha=1.5)):
        with pytest.raises(ValueError):
            back2future.loss_summary(rec, **kw)
    with pytest.raises(ValueError, match="40-word records"):
        back2future.loss_summary(rec[:, :, :32], pme_criterion="SSIM")
    # records of the new width still serve the occlusion-aware summary of their first 16 words, and -no_occ serves the older records
    assert back2future.loss_summary(rec)["mean"] == back2future.loss_summary(rec[:, :, :16])["mean"]
    assert back2future.loss_summary(rec[:, :, :16], no_occ=True)["mean"] < back2future.loss_summary(rec[:, :, :16])["mean"]
