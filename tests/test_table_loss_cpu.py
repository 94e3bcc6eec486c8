"""CPU: the unsupervised validation loss of test.lua:266-297 (include/b2f.h, B2F_LOSS_*) without a GPU: the ABI carries it, the host
entry equals the numpy restatement of the definition on every word, every branch of the record is reached, the library's exponential
stays within 2^-50 of np.exp, loss_summary agrees with a float64 transcription of the reference's criteria within the records'
rounding, and every malformed request is refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_table_loss_host", "b2f_table_loss_device", "b2f_op_table_loss", "b2f_forward_loss", "b2f_forward_loss_device",
           "b2f_multi_forward_loss"]
SHAPES = [(1, 1, 1), (2, 3, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5), (64, 64, 5)]   # (16,16,5): the coarsest level is 1 x 1; (48,80,5): widths 80 .. 5


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


_CASES = {}


def case(H, W, L, past):
    """(table, ref, host records, want records), computed once per shape and kind and left unchanged"""
    key = (H, W, L, past)
    if key not in _CASES:
        table, ref = TL.tables(H, W, L, past)
        _CASES[key] = (table, ref, ops.table_loss(table, ref), TL.want(table, ref, past))
    return _CASES[key]


def test_symbols_enums_and_version_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in cdef and name + "(" in doc, name
    assert _lib.lib().b2f_version() >= 1004
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(B2F_LOSS_\w+) = (\d+)", hdr))
    assert enums == {"B2F_LOSS_PIXELS": 0, "B2F_LOSS_SMOOTH_FLOW_Q30": 1, "B2F_LOSS_SMOOTH_PAST_Q30": 2, "B2F_LOSS_CONST_VEL_Q30": 3,
                     "B2F_LOSS_SMOOTH_OCC_Q30": 4, "B2F_LOSS_PRIOR_OCC_Q30": 5, "B2F_LOSS_PHOTO_INSIDE": 6, "B2F_LOSS_PHOTO_OUTSIDE": 8,
                     "B2F_LOSS_PHOTO_OCHARB_Q30": 10, "B2F_LOSS_PHOTO_NONFINITE": 12, "B2F_LOSS_NONFINITE": 14, "B2F_LOSS_WORDS": 16}
    for k, v in enums.items():
        assert getattr(back2future, k[4:]) == v, k
        assert re.search(r"\b%s = %d\b" % (k, v), doc), k
    assert (TL.WORDS, TL.PIXELS, TL.SMOOTH_FLOW, TL.SMOOTH_PAST, TL.CONST_VEL, TL.SMOOTH_OCC, TL.PRIOR_OCC, TL.INSIDE, TL.OUTSIDE, TL.OCHARB,
            TL.PHOTO_NONFINITE, TL.NONFINITE) == (16, 0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14)
    assert back2future.LOSS_LEVEL_WEIGHTS == TL.LEVEL_WEIGHTS and back2future.LOSS_WEIGHTS == TL.WEIGHTS
    for src in ("back2future_amd/csrc/b2f_tableloss.h", "back2future_amd/csrc/b2f_tableloss.hip"):
        assert "test.lua:266-297" in open(os.path.join(ROOT, src)).read(), src


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_host_entry_equals_the_definition(H, W, L, past):
    table, ref, got, want = case(H, W, L, past)
    assert got.shape == want.shape == (2, L, 16) and got.dtype == np.uint64
    for word in range(16):
        np.testing.assert_array_equal(got[:, :, word], want[:, :, word], err_msg="word %d" % word)
    assert not got[:, :, 15].any()
    if not past:
        assert not got[:, :, TL.SMOOTH_PAST].any() and not got[:, :, TL.CONST_VEL].any()


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_every_pixel_is_counted_once(H, W, L, past):
    got = case(H, W, L, past)[2]
    for j in range(L):
        hw = (H >> j) * (W >> j)
        assert (got[:, j, TL.PIXELS] == hw).all()
        for d in range(2):
            assert (got[:, j, TL.INSIDE + d] + got[:, j, TL.OUTSIDE + d] + got[:, j, TL.PHOTO_NONFINITE + d] == hw).all()


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(37, 53, 1), (48, 80, 5), (64, 64, 5)])
def test_every_branch_is_reached(H, W, L, past):
    got = case(H, W, L, past)[2]
    total = got.reshape(-1, 16).sum(axis=0)
    for word in (TL.OUTSIDE, TL.OUTSIDE + 1, TL.NONFINITE, TL.PHOTO_NONFINITE, TL.PHOTO_NONFINITE + 1, TL.INSIDE, TL.INSIDE + 1, TL.SMOOTH_FLOW,
                 TL.SMOOTH_OCC, TL.PRIOR_OCC, TL.OCHARB, TL.OCHARB + 1):
        assert total[word] > 0, word
    if past:
        assert total[TL.SMOOTH_PAST] > 0 and total[TL.CONST_VEL] > 0


def test_reference_image_has_flat_runs_ramps_and_edges_on_every_level():
    """the contrast weights of the synthetic reference image: exactly 1, strictly between 0 and 1, and about e^-96, on all five levels"""
    ref = TL.reference_image(1, 64, 64, tame=True)
    for R in TL.ref_pyramid(ref, 5):
        dx, dy = TL._diffs(R)
        wx = TL.E(-20.0 * ((np.abs(dx[:, 0]) + np.abs(dx[:, 1])) + np.abs(dx[:, 2])) / 3.0)
        wy = TL.E(-20.0 * ((np.abs(dy[:, 0]) + np.abs(dy[:, 1])) + np.abs(dy[:, 2])) / 3.0)
        assert (wy[..., :-1, :] == 1.0).any() and ((wy[..., :-1, :] > 1e-3) & (wy[..., :-1, :] < 0.9)).any()
        assert ((wx > 0) & (wx < 1e-30)).any()


def test_exponential_against_numpy():
    t = np.concatenate([np.linspace(-708.0, 0.0, 600001), -np.logspace(-300, 2.8, 2000), [0.0, -0.0, -708.0]])
    got, ref = TL.E(t), np.exp(t)
    assert np.abs(got / ref - 1.0).max() <= 2.0 ** -50
    assert TL.E(np.array([-708.5, -1e9, -np.inf])).tolist() == [0.0, 0.0, 0.0]
    assert TL.E(np.array([3.0]))[0] == 1.0 and np.isnan(TL.E(np.array([np.nan]))[0])


def test_host_exponential_is_the_restatement():
    """The host entry's E against the numpy one through a table: a flat flow (every P1 term is exactly sqrt(1e-6)) over a ramp image
    makes the smoothness word a function of the two weights alone."""
    H, W = 8, 64
    slopes = np.linspace(0.0, 34.0, W, dtype=np.float32)          # t = -20 * slope down to about -680
    ref = np.cumsum(slopes)[None, None, None, :].repeat(3, 1).repeat(H, 2).astype(np.float32)
    table = [np.zeros((1, 2, H, W), np.float32), np.full((1, 2, H, W), 0.5, np.float32), np.zeros((1, 3, H, W), np.float32),
             np.zeros((1, 3, H, W), np.float32)]
    np.testing.assert_array_equal(ops.table_loss(table, ref), TL.want(table, ref, False))


@pytest.mark.parametrize("size_average", [False, True], ids=["sum", "size_average"])
@pytest.mark.parametrize("like", ["test", "train"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(37, 53, 1), (48, 80, 5), (64, 96, 5)])
def test_loss_summary_against_the_lua_criteria(H, W, L, past, like, size_average):
    """|loss - lua_loss| <= sum over levels and terms of level_weight * weight * h w * 2^-31 + 1e-12 |lua_loss| (table_loss_fields.bound):
    the bar is the records' rounding, not a tuned figure."""
    table, ref = TL.tables(H, W, L, past, tame=True)
    rec = ops.table_loss(table, ref)
    s = back2future.loss_summary(rec, like=like, size_average=size_average)
    assert s["nonfinite"] == 0
    per = 5 if past else 4
    for j in range(L):      # the 0-based fp32 mask of the record and the 1-based one of OBCCriterion.lua:97-100 agree on every pixel
        k = float(np.float32(TL.SCALE / 2.0 ** j))
        for d, fl in enumerate((table[j * per + (1 if past else 0)], table[j * per])):
            zero_based, one_based = TL.inside_masks(fl, -k if d == 0 else k)
            assert (zero_based == one_based).all(), (j, d)
    lua = TL.lua_loss(table, ref, past, like=like, size_average=size_average)
    assert s["loss"].shape == lua.shape == (2,)
    for b in range(2):
        bar = TL.bound(H, W, L, past, like=like, size_average=size_average, lua=lua[b])
        print("H %d W %d L %d past %d %s avg %d image %d: loss %.12g lua %.12g diff %.3g bar %.3g" % (H, W, L, past, like, size_average, b, s["loss"][b],
                                                                                              lua[b], abs(s["loss"][b] - lua[b]), bar))
        assert abs(s["loss"][b] - lua[b]) <= bar
    assert s["mean"] == pytest.approx(float(s["loss"].mean()), rel=1e-15)
    assert s["level"].shape == (2, L) and np.allclose(s["level"].sum(axis=1), s["loss"], rtol=1e-14)


def test_loss_summary_weights_and_shapes():
    table, ref = TL.tables(16, 16, 2, True, tame=True)
    rec = ops.table_loss(table, ref)
    wts = {"smooth_flow": 0.5, "const_vel": 2.0, "pme": 3.0, "smooth_occ": 0.0, "prior_occ": 1.0}
    s, lua = back2future.loss_summary(rec, weights=wts), TL.lua_loss(table, ref, True, weights=wts)
    for b in range(2):
        assert abs(s["loss"][b] - lua[b]) <= TL.bound(16, 16, 2, True, weights=wts, lua=lua[b])
    one = back2future.loss_summary(rec[0])
    assert one["loss"].shape == (1,) and one["loss"][0] == back2future.loss_summary(rec)["loss"][0]
    with pytest.raises(ValueError):
        back2future.loss_summary(rec.astype(np.int64))
    with pytest.raises(ValueError):
        back2future.loss_summary(rec, like="eval")


def _host(table, n_outs, n, H, W, past, ref, scale=20.0, loss=True):
    ptrs = (_lib.c_float_p * max(len(table), 1))(*[_lib.fptr(t) if t is not None else None for t in table]) if table is not None else None
    out = np.zeros((max(n, 1), 8, 16), np.uint64)
    return _lib.lib().b2f_table_loss_host(ptrs, n_outs, n, H, W, past, _lib.fptr(ref) if ref is not None else None, scale,
                                          out.ctypes.data_as(C.POINTER(C.c_ulonglong)) if loss else None)


def test_refusals_need_no_gpu():
    z = lambda c, h, w: np.zeros((1, c, h, w), np.float32)
    level = lambda h, w, past: [z(2, h, w)] * (3 if past else 2) + [z(3, h, w)] * 2
    ref = z(3, 16, 16)
    good = level(16, 16, False)
    assert _host(good, 4, 1, 16, 16, 0, ref) == 0
    last = lambda: _lib.lib().b2f_last_error().decode()
    assert _host(good, 0, 1, 16, 16, 0, ref) != 0 and "n_outs" in last()                    # L = 0
    eight = sum([level(128 >> j, 128 >> j, False) for j in range(8)], [])
    assert _host(eight, 32, 1, 128, 128, 0, z(3, 128, 128)) != 0 and "1 .. 7 levels" in last()   # L = 8
    two = level(18, 16, False) + level(9, 8, False)
    assert _host(two, 8, 1, 18, 16, 0, z(3, 18, 16)) == 0
    three = two + level(4, 4, False)
    assert _host(three, 12, 1, 18, 16, 0, z(3, 18, 16)) != 0 and "multiples of 2^(L - 1)" in last()   # 18 is no multiple of 4
    assert _host(three, 12, 1, 16, 18, 0, z(3, 16, 18)) != 0 and "multiples of 2^(L - 1)" in last()
    assert _host(good + good[:3], 7, 1, 16, 16, 0, ref) != 0 and "n_outs" in last()         # fits neither kind
    assert _host(good + good[:3], 7, 1, 16, 16, 1, ref) != 0 and "n_outs" in last()
    assert _host(good, 4, 1, 16, 16, 1, ref) != 0                                            # a Hard table read as Soft
    assert _host(None, 4, 1, 16, 16, 0, ref) != 0 and "null" in last()
    assert _host(good, 4, 1, 16, 16, 0, None) != 0 and "null" in last()
    assert _host(good, 4, 1, 16, 16, 0, ref, loss=False) != 0 and "null" in last()
    assert _host(good[:3] + [None], 4, 1, 16, 16, 0, ref) != 0 and "null" in last()
    assert _host(good, 4, 0, 16, 16, 0, ref) != 0 and _host(good, 4, 1, 0, 16, 0, ref) != 0
    assert _host(good, 4, 1, 1 << 14, 1 << 14, 0, ref) != 0 and "2^28" in last()            # refused before anything is read
    for bad in (0.0, -20.0, float("nan"), float("inf")):
        assert _host(good, 4, 1, 16, 16, 0, ref, scale=bad) != 0 and "flow_scale" in last()
    with pytest.raises(ValueError):
        ops.table_loss(good[:3], ref)
    with pytest.raises(ValueError):
        ops.table_loss(level(8, 16, False), ref)
