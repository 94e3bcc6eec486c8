"""CPU: the fine-tuning objective of the Soft models (README.md:89-102; include/b2f.h, B2F_LOSS_FT_*) without a GPU: the host entry
keeps words 0 .. 15 of b2f_table_loss_host, its words 16 .. 23 equal the numpy restatement of the definition, loss_summary agrees
with a float64 transcription of SecondOrderSmoothnessCriterion and OBGCCriterion within the records' rounding, a border pixel adds
P1(0) = 1e-3 times its weight, and malformed requests are refused.  (The exponent of the new weight goes through the library's E,
which tests/test_table_loss_cpu.py holds against np.exp.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL
from tests import table_loss_ft_fields as FT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_table_loss_ft_host", "b2f_table_loss_ft_device", "b2f_op_table_loss_ft", "b2f_forward_loss_ft", "b2f_forward_loss_ft_device",
           "b2f_multi_forward_loss_ft"]
# (16,16,5): the coarsest level is 1 x 1; (48,80,5): widths 80 .. 5; the small ones: maps the reference cannot slice
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


_CASES = {}


def case(H, W, L, past, scale):
    """(table, ref, host records of 24 words, host records of 16 words, want words 16 .. 23), computed once and left unchanged"""
    key = (H, W, L, past, scale)
    if key not in _CASES:
        table, ref = TL.tables(H, W, L, past)
        _CASES[key] = (table, ref, ops.table_loss(table, ref, flow_scale=scale, objective="finetune"), ops.table_loss(table, ref, flow_scale=scale),
                       FT.want_ft(table, ref, past, flow_scale=scale))
    return _CASES[key]


def test_entries_and_words_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_ft", "")], name      # the same argument lists
        assert name + "(" in cdef and name + "(" in doc, name
    assert _lib.lib().b2f_version() >= 1006
    words = dict((k, int(v)) for k, v in re.findall(r"#define (B2F_LOSS_FT_\w+) (\d+)", hdr))
    assert words == {"B2F_LOSS_FT_SMOOTH2_FLOW_Q30": 16, "B2F_LOSS_FT_SMOOTH2_PAST_Q30": 17, "B2F_LOSS_FT_PHOTO_OGX_Q30": 18,
                     "B2F_LOSS_FT_PHOTO_OGY_Q30": 20, "B2F_LOSS_FT_SMOOTH2_NONFINITE": 22, "B2F_LOSS_FT_GRAD_NONFINITE": 23,
                     "B2F_LOSS_FT_WORDS": 24}
    for k, v in words.items():
        assert getattr(back2future, k[4:]) == v, k
        assert re.search(r"\b%s %d\b" % (k, v), doc), k
    assert (FT.WORDS, FT.SMOOTH2_FLOW, FT.SMOOTH2_PAST, FT.OGX, FT.OGY, FT.SMOOTH2_NONFINITE, FT.GRAD_NONFINITE) == (24, 16, 17, 18, 20, 22, 23)
    assert sorted(back2future.LOSS_OBJECTIVES) == sorted(FT.OBJECTIVES) == ["Ours-Hard", "Ours-Soft-ft-KITTI", "Ours-Soft-ft-Sintel"]
    for name, o in FT.OBJECTIVES.items():
        got = back2future.LOSS_OBJECTIVES[name]
        assert (got["weights"], got["smooth_second_order"], got["pme_criterion"], got["pme_beta"], got["pme_gamma"], got["past_flow"]) == \
               (o["weights"], o["second"], o["criterion"], o["beta"], o["gamma"], o["past"]), name


@pytest.mark.parametrize("scale", [20.0, 10.0])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_words_0_to_15_are_the_existing_records(H, W, L, past, scale):
    _, _, got, base, _ = case(H, W, L, past, scale)
    assert got.shape == (2, L, 24) and got.dtype == np.uint64 and base.shape == (2, L, 16)
    np.testing.assert_array_equal(got[:, :, :16], base)


@pytest.mark.parametrize("scale", [20.0, 10.0])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_words_16_to_23_equal_the_definition(H, W, L, past, scale):
    _, _, got, _, want = case(H, W, L, past, scale)
    for word in range(16, 24):
        np.testing.assert_array_equal(got[:, :, word], want[:, :, word - 16], err_msg="word %d" % word)
    if not past:
        assert not got[:, :, FT.SMOOTH2_PAST].any()
    assert (got[:, :, FT.SMOOTH2_FLOW] > 0).all()          # even a 1 x 1 level adds P1(0) twice per channel


def test_both_nonfinite_words_are_reached():
    total = np.zeros(24, np.uint64)
    for H, W, L in SHAPES:
        for past in (False, True):
            for scale in (20.0, 10.0):
                total += case(H, W, L, past, scale)[2].reshape(-1, 24).sum(axis=0)
    assert total[FT.SMOOTH2_NONFINITE] > 0 and total[FT.GRAD_NONFINITE] > 0
    for word in (FT.SMOOTH2_FLOW, FT.SMOOTH2_PAST, FT.OGX, FT.OGX + 1, FT.OGY, FT.OGY + 1):
        assert total[word] > 0, word


@pytest.mark.parametrize("like", ["test", "train"])
@pytest.mark.parametrize("name", sorted(FT.OBJECTIVES))
@pytest.mark.parametrize("H,W,L", [(37, 53, 1), (48, 80, 5), (64, 96, 5)])
def test_loss_summary_against_the_lua_criteria(H, W, L, name, like):
    """|loss - lua_loss_ft| <= sum over levels and terms of level_weight * weight * pixel terms * 2^-31 + 1e-12 |lua|
    (table_loss_ft_fields.bound_ft): the bar is the records' rounding, derived and not measured."""
    o = FT.OBJECTIVES[name]
    past = o["past"]
    table, ref = TL.tables(H, W, L, past, tame=True)
    rec = ops.table_loss(table, ref, objective="finetune")
    assert not rec[:, :, [TL.NONFINITE, TL.PHOTO_NONFINITE, TL.PHOTO_NONFINITE + 1, FT.SMOOTH2_NONFINITE, FT.GRAD_NONFINITE]].any()
    s = back2future.loss_summary(rec, like=like, objective=name)
    assert s["nonfinite"] == 0
    per = 5 if past else 4
    for j in range(L):      # the 0-based fp32 mask of the record and the 1-based one of OBGCCriterion.lua:127-130 agree on every pixel
        k = float(np.float32(TL.SCALE / 2.0 ** j))
        for d, fl in enumerate((table[j * per + (1 if past else 0)], table[j * per])):
            zero_based, one_based = TL.inside_masks(fl, -k if d == 0 else k)
            assert (zero_based == one_based).all(), (j, d)
    lua = FT.lua_loss_ft(table, ref, past, like=like, second=o["second"], criterion=o["criterion"], beta=o["beta"], gamma=o["gamma"],
                         weights=o["weights"])
    assert s["loss"].shape == lua.shape == (2,)
    for b in range(2):
        bar = FT.bound_ft(H, W, L, past, second=o["second"], criterion=o["criterion"], beta=o["beta"], gamma=o["gamma"], weights=o["weights"], lua=lua[b])
        diff = abs(s["loss"][b] - lua[b])
        print("H %d W %d L %d %s %s image %d: loss %.12g lua %.12g diff %.3g bar %.3g ratio %.3g" % (H, W, L, name, like, b, s["loss"][b], lua[b], diff,
                                                                                                bar, diff / bar))
        assert diff <= bar
    # the same options spelled out, and with the norms of -sizeAverage
    kw = dict(smooth_second_order=o["second"], pme_criterion=o["criterion"], pme_beta=o["beta"], pme_gamma=o["gamma"]) if o["criterion"] == "OBGCC" else {}
    t = back2future.loss_summary(rec, like=like, weights=o["weights"], **kw)
    assert np.array_equal(t["loss"], s["loss"])
    t = back2future.loss_summary(rec, like=like, size_average=True, weights=o["weights"], **kw)
    lua = FT.lua_loss_ft(table, ref, past, like=like, size_average=True, second=o["second"], criterion=o["criterion"], beta=o["beta"],
                         gamma=o["gamma"], weights=o["weights"])
    for b in range(2):
        assert abs(t["loss"][b] - lua[b]) <= FT.bound_ft(H, W, L, past, second=o["second"], criterion=o["criterion"], beta=o["beta"], gamma=o["gamma"], size_average=True,
                                                         weights=o["weights"], lua=lua[b])


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_a_border_pixel_adds_p1_of_zero(past):
    """A constant flow over a constant reference image: every second difference is 0 and every weight 1, so each of the h w pixels
    adds P1(0) = 1e-3 for two axes and two channels: 2 h w 2 1e-3 per flow and level, within 2^-31 per rounded product, four a pixel.  A pixel that added
    nothing on the border (first and last column and row) would leave the sum short by 1e-3 per axis and channel."""
    H, W, L = 12, 20, 3
    table = []
    for j in range(L):
        h, w = H >> j, W >> j
        table += [np.full((1, 2, h, w), 0.25, np.float32)] * (2 if past else 1) + [np.full((1, 2, h, w), 0.5, np.float32)]
        table += [np.zeros((1, 3, h, w), np.float32)] * 2
    rec = ops.table_loss(table, np.full((1, 3, H, W), 0.75, np.float32), objective="finetune")
    for j in range(L):
        hw = (H >> j) * (W >> j)
        for word in [FT.SMOOTH2_FLOW] + ([FT.SMOOTH2_PAST] if past else []):
            got = float(rec[0, j, word]) / 2.0 ** 30
            assert abs(got - 2 * hw * 2 * 1e-3) <= 4 * hw * 2.0 ** -31 + 1e-15 * hw, (j, word, got)
    if not past:
        assert not rec[:, :, FT.SMOOTH2_PAST].any()
    assert not rec[:, :, FT.SMOOTH2_NONFINITE].any()


def test_argument_errors():
    table, ref = TL.tables(16, 16, 2, True, tame=True)
    rec16, rec24 = ops.table_loss(table, ref), ops.table_loss(table, ref, objective="finetune")
    for kw in ({"pme_criterion": "OBGCC"}, {"smooth_second_order": True}, {"pme_beta": 0.5}, {"pme_gamma": 0.0},
               {"objective": "Ours-Soft-ft-KITTI"}, {"objective": "Ours-Soft-ft-Sintel"}):
        with pytest.raises(ValueError):
            back2future.loss_summary(rec16, **kw)
        back2future.loss_summary(rec24, **kw)
    assert back2future.loss_summary(rec16, objective="Ours-Hard")["loss"].shape == (2,)
    # a 24-word record with the default arguments is the 16-word summary
    a, b = back2future.loss_summary(rec24), back2future.loss_summary(rec16)
    assert np.array_equal(a["loss"], b["loss"]) and a["nonfinite"] == b["nonfinite"]
    with pytest.raises(ValueError):
        back2future.loss_summary(rec24, objective="Ours-Soft")
    with pytest.raises(ValueError):
        back2future.loss_summary(rec24, objective="Ours-Soft-ft-KITTI", pme_beta=0.5)
    with pytest.raises(ValueError):
        back2future.loss_summary(rec24, pme_criterion="SSIM")
    with pytest.raises(ValueError):
        back2future.loss_summary(rec24[:, :, :20])
    with pytest.raises(ValueError):
        ops.table_loss(table, ref, objective="train")
    with pytest.raises(ValueError):
        ops.table_loss(table, ref, objective=None)


def test_the_host_entry_refuses_what_the_existing_one_refuses():
    z = lambda c, h, w: np.zeros((1, c, h, w), np.float32)
    good = [z(2, 16, 16)] * 2 + [z(3, 16, 16)] * 2
    ref = z(3, 16, 16)
    out = np.full((1, 1, 24), 7, np.uint64)

    def host(table, n_outs, n, H, W, past, scale=20.0):
        ptrs = (_lib.c_float_p * len(table))(*[_lib.fptr(t) if t is not None else None for t in table])
        return _lib.lib().b2f_table_loss_ft_host(ptrs, n_outs, n, H, W, past, _lib.fptr(ref), scale, out.ctypes.data_as(C.POINTER(C.c_ulonglong)))

    last = lambda: _lib.lib().b2f_last_error().decode()
    assert host(good, 0, 1, 16, 16, 0) != 0 and "n_outs" in last() and "b2f_table_loss_ft_host" in last()
    assert host(good, 4, 1, 16, 16, 1) != 0
    assert host(good[:3] + [None], 4, 1, 16, 16, 0) != 0 and "null" in last()
    assert host(good, 4, 1, 16, 16, 0, scale=0.0) != 0 and "flow_scale" in last()
    assert (out == 7).all()                                  # nothing written by a refused call
    assert host(good, 4, 1, 16, 16, 0) == 0 and out[0, 0, 0] == 256 and out[0, 0, 15] == 0
