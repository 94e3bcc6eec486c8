"""CPU: the occlusion-aware SSIM + L1 photometric term (criterions/OSSIML1Criterion.lua; include/b2f.h, B2F_LOSS_SSIM_*) without a GPU:
the host entry keeps words 0 .. 15 of b2f_table_loss_host, its words 16 .. 25 equal the numpy restatement of the definition in the
three range modes with no tolerance, loss_summary agrees with a float64 transcription of OSSIML1Criterion:updateOutput (another
window: a 2-D kernel from the Gaussian formula, torch's replicate padding and conv2d) within the records' rounding plus the derived
float64 evaluation error of that transcription, the exact cases of the definition hold, four wrong readings of it are told from the
right one, and malformed requests are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_fields as TL
from tests import table_loss_ssim_fields as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_table_loss_ssim_host", "b2f_table_loss_ssim_device", "b2f_op_table_loss_ssim", "b2f_forward_loss_ssim", "b2f_forward_loss_ssim_device",
           "b2f_multi_forward_loss_ssim"]
# (16,16,5): the coarsest level is 1 x 1; (48,80,5): widths 80 .. 5; the small ones: levels whose windows are mostly replication
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
MODES = ["batch", "image", "given"]
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def given(L):
    """a range per level that holds the fields' values without being anyone's own"""
    return np.array([[-3.0 - 0.25 * j, 3.5 + 0.125 * j] for j in range(L)], F32)


def fields(H, W, L, past, tame=False):
    """the tables of table_loss_fields with the second image at half the values: the batch's range is not each image's own"""
    table, ref = TL.tables(H, W, L, past, tame=tame)
    table = [t.copy() for t in table]
    per = 5 if past else 4
    for i, t in enumerate(table):
        if i % per >= per - 2:
            t[1] *= F32(0.5)
    return table, ref


_CASES = {}


def case(H, W, L, past, scale, mode):
    """(table, ref, host records of 32 words, host records of 16 words, want words 16 .. 25), computed once and left unchanged"""
    key = (H, W, L, past, scale, mode)
    if key not in _CASES:
        table, ref = fields(H, W, L, past)
        rng = given(L) if mode == "given" else mode
        _CASES[key] = (table, ref, ops.table_loss(table, ref, flow_scale=scale, objective="ssim", ssim_range=rng), ops.table_loss(table, ref, flow_scale=scale),
                       SS.want_ssim(table, ref, past, flow_scale=scale, mode=MODES.index(mode), ranges=given(L)))
    return _CASES[key]


def test_entries_and_words_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES + ["b2f_loss_ssim_weights"]:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in cdef and name + "(" in doc, name
    for name in ENTRIES:       # the argument list of the _ft sibling plus (int range_mode, const float *ranges)
        assert _lib.SIGNATURES[name] == (C.c_int, _lib.SIGNATURES[name.replace("_ssim", "_ft")][1] + [C.c_int, _lib.c_float_p]), name
    assert _lib.lib().b2f_version() >= 1010
    words = dict((k, int(v)) for k, v in re.findall(r"#define (B2F_LOSS_SSIM_\w+) (\d+)", hdr))
    assert words == {"B2F_LOSS_SSIM_Q30": 16, "B2F_LOSS_SSIM_L1N_Q30": 18, "B2F_LOSS_SSIM_NONFINITE": 20, "B2F_LOSS_SSIM_RANGE_USED": 22,
                     "B2F_LOSS_SSIM_RANGE_OWN": 24, "B2F_LOSS_SSIM_WORDS": 32}
    for k, v in words.items():
        assert getattr(back2future, k[4:]) == v, k
        assert re.search(r"\b%s %d\b" % (k, v), doc), k
    modes = dict((k, int(v)) for k, v in re.findall(r"#define (B2F_SSIM_RANGE_\w+) (\d+)", hdr))
    assert modes == {"B2F_SSIM_RANGE_BATCH": 0, "B2F_SSIM_RANGE_IMAGE": 1, "B2F_SSIM_RANGE_GIVEN": 2}
    assert (back2future.SSIM_RANGE_BATCH, back2future.SSIM_RANGE_IMAGE, back2future.SSIM_RANGE_GIVEN) == (SS.BATCH, SS.IMAGE, SS.GIVEN) == (0, 1, 2)
    assert (SS.WORDS, SS.SSIM, SS.L1N, SS.SSIM_NONFINITE, SS.RANGE_USED, SS.RANGE_OWN) == (32, 16, 18, 20, 22, 24)
    assert back2future.loss_words("ssim") == 32 and back2future.loss_words("finetune") == 24 and back2future.loss_words("pme") == 16
    assert back2future.SSIM_ALPHA == SS.ALPHA == {"OSSIM": 1.0, "OSSIML1": 0.85}
    assert "B2F_LOSS_WORDS = 16" in hdr                           # the enumeration stays as it is


def test_the_window_is_the_normalised_gaussian_of_the_formula():
    """ge = e / (1 + 2 e), gc = 1 / (1 + 2 e), e = exp(-8/9); their outer product is the 2-D kernel the transcription builds from the
    Gaussian formula, to a few units in the last place."""
    ge, gc = SS.weights()
    e = np.exp(-8.0 / 9.0)
    assert abs(ge - e / (1 + 2 * e)) <= 2.0 ** -53 and abs(gc - 1 / (1 + 2 * e)) <= 2.0 ** -53
    assert abs(2 * ge + gc - 1.0) <= 2.0 ** -52
    k = np.outer([ge, gc, ge], [ge, gc, ge])
    assert np.abs(k - SS.gaussian3()).max() <= 4 * 2.0 ** -53


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", [20.0, 10.0])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", SHAPES)
def test_the_words_equal_the_existing_records_and_the_definition(H, W, L, past, scale, mode):
    _, _, got, base, want = case(H, W, L, past, scale, mode)
    assert got.shape == (2, L, 32) and got.dtype == np.uint64 and base.shape == (2, L, 16)
    np.testing.assert_array_equal(got[:, :, :16], base)
    for word in range(16, 26):
        np.testing.assert_array_equal(got[:, :, word], want[:, :, word - 16], err_msg="word %d" % word)
    assert not got[:, :, 26:].any()
    if mode == "given":
        assert (got[:, :, SS.RANGE_USED:SS.RANGE_USED + 2].astype(np.uint32).view(F32) == given(L)[None]).all()


def test_the_range_words():
    """Words 24 / 25 are the same in every mode; batch mode on two images with different ranges differs from image mode; the batch's
    words 22 / 23 are the minimum of the minima and the maximum of the maxima; GIVEN with them reproduces BATCH bit for bit; batch mode
    on one image equals image mode."""
    reached = False
    for H, W, L in SHAPES:
        for past in (False, True):
            table, ref, b, _, _ = case(H, W, L, past, 20.0, "batch")
            i = case(H, W, L, past, 20.0, "image")[2]
            g = case(H, W, L, past, 20.0, "given")[2]
            np.testing.assert_array_equal(b[:, :, 24:26], i[:, :, 24:26])
            np.testing.assert_array_equal(b[:, :, 24:26], g[:, :, 24:26])
            np.testing.assert_array_equal(i[:, :, 22:24], i[:, :, 24:26])
            own = i[:, :, 24:26].astype(np.uint32).view(F32)
            used = b[:, :, 22:24].astype(np.uint32).view(F32)
            assert (used[:, :, 0] == np.nanmin(own[:, :, 0], axis=0)[None]).all() and (used[:, :, 1] == np.nanmax(own[:, :, 1], axis=0)[None]).all()
            again = ops.table_loss(table, ref, objective="ssim", ssim_range=used[0])
            np.testing.assert_array_equal(again, b)
            for img in range(2):    # an image that sums anything and whose own range is not the batch's
                if i[img, :, 16:20].any() and not np.array_equal(own[img], used[img]):
                    reached = True
                    assert not np.array_equal(b[img, :, 16:20], i[img, :, 16:20]), (H, W, L, past, img)
            one = [t[:1] for t in table]
            np.testing.assert_array_equal(ops.table_loss(one, ref[:1], objective="ssim", ssim_range="batch"),
                                          ops.table_loss(one, ref[:1], objective="ssim", ssim_range="image"))
            np.testing.assert_array_equal(ops.table_loss(one, ref[:1], objective="ssim", ssim_range="image"), i[:1])     # cut-invariant
    assert reached


def test_every_word_is_reached():
    total = np.zeros(32, np.uint64)
    for H, W, L in SHAPES:
        for past in (False, True):
            total += case(H, W, L, past, 20.0, "batch")[2].reshape(-1, 32).sum(axis=0)
    for word in range(16, 22):
        assert total[word] > 0, word


@pytest.mark.parametrize("mutation", SS.MUTATIONS)
@pytest.mark.parametrize("H,W", [(1, 5), (3, 3)])
def test_a_wrong_reading_of_the_definition_is_told_from_the_right_one(H, W, mutation):
    """zero padding instead of replication, ge and gc swapped, the occlusion channel of the other direction, the L1 penalty of the
    difference before normalisation: each changes words 16 .. 19 of the restatement on these two small levels, so the comparison with
    no tolerance above is red for a library that reads the definition that way."""
    for past in (False, True):
        table, ref, got, _, want = case(H, W, 1, past, 20.0, "batch")
        wrong = SS.want_ssim(table, ref, past, mode=SS.BATCH, mutation=mutation)
        assert np.array_equal(got[:, :, 16:26], want)
        assert not np.array_equal(wrong[:, :, :4], want[:, :, :4]), (mutation, past)


def _plain_table(H, W, L, past, iw, occ=0.5):
    """zero flows (every target inside), constant occlusions, the same warped image in both directions: iw(j) -> 1 x 3 x h x w"""
    table = []
    for j in range(L):
        h, w = H >> j, W >> j
        table += [np.zeros((1, 2, h, w), F32)] * (2 if past else 1) + [np.full((1, 2, h, w), occ, F32)]
        table += [iw(j).copy(), iw(j).copy()]
    return table


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_exact_cases(past):
    H, W, L = 12, 20, 3
    r = np.random.default_rng(5)
    ref = r.uniform(-2, 2, (1, 3, H, W)).astype(F32)
    pyr = TL.ref_pyramid(ref, L)
    # warped images equal to the reference: l = cs = 1 exactly in this arithmetic, so 1 - l cs = 0 on every pixel
    rec = ops.table_loss(_plain_table(H, W, L, past, lambda j: pyr[j]), ref, objective="ssim", ssim_range="image")
    hw = np.array([(H >> j) * (W >> j) for j in range(L)], np.uint64)
    assert (rec[0, :, TL.INSIDE] == hw).all() and (rec[0, :, TL.INSIDE + 1] == hw).all()
    assert not rec[:, :, SS.SSIM:SS.SSIM + 2].any() and not rec[:, :, SS.SSIM_NONFINITE:SS.SSIM_NONFINITE + 2].any()
    # ... and the L1 word is o * 3 * P1(0) = 0.5 * 3e-3 per pixel-direction, each rounded by at most 2^-31
    for j in range(L):
        for d in range(2):
            assert abs(float(rec[0, j, SS.L1N + d]) / 2.0 ** 30 - 1.5e-3 * float(hw[j])) <= float(hw[j]) * (2.0 ** -31 + 1e-18)
    # a constant image under a given range: zero as well
    flat = np.full((1, 3, H, W), 0.75, F32)
    rec = ops.table_loss(_plain_table(H, W, L, past, lambda j: np.full((1, 3, H >> j, W >> j), 0.75, F32)), flat, objective="ssim",
                         ssim_range=np.array([[0.0, 1.0]] * L, F32))
    assert not rec[:, :, SS.SSIM:SS.SSIM + 2].any() and not rec[:, :, SS.SSIM_NONFINITE:SS.SSIM_NONFINITE + 2].any() and rec[:, :, SS.L1N].all()
    # the same table on its own range: all nine planes constant, mx == mn: every inside pixel-direction is non-finite, nothing is summed
    for rng in ("image", "batch"):
        rec = ops.table_loss(_plain_table(H, W, L, past, lambda j: np.full((1, 3, H >> j, W >> j), 0.75, F32)), flat, objective="ssim", ssim_range=rng)
        assert not rec[:, :, SS.SSIM:SS.SSIM + 4].any()
        assert (rec[0, :, SS.SSIM_NONFINITE] == hw).all() and (rec[0, :, SS.SSIM_NONFINITE + 1] == hw).all()
        assert (rec[0, :, 22:26].astype(np.uint32).view(F32) == F32(0.75)).all()
    # a range that is not finite, or upside down
    for bad in ([0.0, np.inf], [np.nan, 1.0], [1.0, 0.0], [1.0, 1.0]):
        rec = ops.table_loss(_plain_table(H, W, 1, past, lambda j: pyr[0]), ref, objective="ssim", ssim_range=np.array([bad], F32))
        assert not rec[:, :, SS.SSIM:SS.SSIM + 4].any() and (rec[0, 0, SS.SSIM_NONFINITE:SS.SSIM_NONFINITE + 2] == hw[0]).all(), bad
    # planes of NaNs alone have no range: words 24 / 25 are NaNs and every inside pixel-direction ... is none: the photo term is NaN too
    nan = np.full((1, 3, 4, 4), np.nan, F32)
    rec = ops.table_loss(_plain_table(4, 4, 1, past, lambda j: nan), nan, objective="ssim", ssim_range="image")
    assert np.isnan(rec[0, 0, 24:26].astype(np.uint32).view(F32)).all() and not rec[:, :, 16:22].any()


@pytest.mark.parametrize("y,x,windows", [(5, 7, 9), (0, 0, 4), (0, 9, 6), (11, 19, 4), (6, 0, 6)])
def test_a_nan_in_one_warped_pixel_moves_the_pixel_directions_whose_window_holds_it(y, x, windows):
    """Every target inside, a given range (the NaN is skipped by the own range, which could move otherwise).  The windows that hold
    pixel (y, x) are those of its 3 x 3 neighbourhood in the plane: nine, six at an edge, four in a corner.  The pixel itself leaves
    PHOTO_INSIDE for PHOTO_NONFINITE (its brightness term is NaN), the others move from the SSIM sums to SSIM_NONFINITE; the other
    direction does not change."""
    H, W = 12, 20
    r = np.random.default_rng(6)
    ref = r.uniform(-2, 2, (1, 3, H, W)).astype(F32)
    iw = r.uniform(-2, 2, (1, 3, H, W)).astype(F32)
    rng = np.array([[-2.5, 2.5]], F32)
    table = _plain_table(H, W, 1, False, lambda j: iw)
    clean = ops.table_loss(table, ref, objective="ssim", ssim_range=rng)
    table[2][0, 1, y, x] = np.nan                                  # warped image 1, channel 1
    rec = ops.table_loss(table, ref, objective="ssim", ssim_range=rng)
    assert rec[0, 0, TL.PHOTO_NONFINITE] == 1 and rec[0, 0, TL.INSIDE] == H * W - 1
    assert rec[0, 0, SS.SSIM_NONFINITE] == windows - 1 and rec[0, 0, SS.SSIM_NONFINITE + 1] == 0
    for word in (SS.SSIM + 1, SS.L1N + 1, TL.INSIDE + 1):
        assert rec[0, 0, word] == clean[0, 0, word]
    assert rec[0, 0, SS.SSIM] < clean[0, 0, SS.SSIM] and rec[0, 0, SS.L1N] < clean[0, 0, SS.L1N]
    np.testing.assert_array_equal(rec[:, :, 16:26], SS.want_ssim(table, ref, False, mode=SS.GIVEN, ranges=rng))
    np.testing.assert_array_equal(rec[0, 0, 24:26], clean[0, 0, 24:26])   # the own range skips the NaN


@pytest.mark.parametrize("like", ["test", "train"])
@pytest.mark.parametrize("criterion", ["OSSIM", "OSSIML1"])
@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(37, 53, 1), (48, 80, 5), (64, 96, 5)])
def test_loss_summary_against_the_lua_criterion(H, W, L, past, criterion, like):
    """|loss - lua_loss_ssim| <= bound_ssim + allowance_ssim: the records' rounding (2^-31 per q and counted pixel-direction, scaled as
    the summary scales it, and every other term's as in table_loss_fields.bound, with 1e-12 |lua| for the float64 sums of the
    transcription) plus what two correct float64 evaluations of 1 - l cs in different orders may differ by (derived in
    table_loss_ssim_fields.allowance_ssim from C1 = 1e-4 and C2 = 9e-4 under the divisions; about 2.9e-10 per counted pixel-direction
    and unit of alpha).  Nothing of the bar is measured on the library.  Batch range: the reference's own rule on the two triplets as
    one batch; image range: each triplet a batch of one."""
    table, ref = fields(H, W, L, past, tame=True)
    alpha = SS.ALPHA[criterion]
    for rng, batch in (("batch", True), ("image", False)):
        rec = ops.table_loss(table, ref, objective="ssim", ssim_range=rng)
        assert not rec[:, :, [TL.NONFINITE, TL.PHOTO_NONFINITE, TL.PHOTO_NONFINITE + 1, SS.SSIM_NONFINITE, SS.SSIM_NONFINITE + 1]].any()
        s = back2future.loss_summary(rec, like=like, pme_criterion=criterion)
        assert s["nonfinite"] == 0
        per = 5 if past else 4
        for j in range(L):      # the 0-based fp32 mask of the record and the 1-based one of OSSIML1Criterion.lua:141-144 agree on every pixel
            k = float(F32(TL.SCALE / 2.0 ** j))
            for d, fl in enumerate((table[j * per + (1 if past else 0)], table[j * per])):
                zero_based, one_based = TL.inside_masks(fl, -k if d == 0 else k)
                assert (zero_based == one_based).all(), (j, d)
        for size_average in (False, True):
            t = back2future.loss_summary(rec, like=like, pme_criterion=criterion, size_average=size_average)
            lua = SS.lua_loss_ssim(table, ref, past, criterion=criterion, like=like, size_average=size_average, batch=batch)
            assert t["loss"].shape == lua.shape == (2,)
            for b in range(2):
                bar = SS.bound_ssim(H, W, L, past, alpha, like=like, size_average=size_average, lua=lua[b]) + SS.allowance_ssim(H, W, L, alpha, size_average)
                diff = abs(t["loss"][b] - lua[b])
                print("H %d W %d L %d %s %s %s %s avg %d image %d: loss %.12g lua %.12g diff %.3g bar %.3g share %.3g" % (
                    H, W, L, "soft" if past else "hard", criterion, like, rng, size_average, b, t["loss"][b], lua[b], diff, bar, diff / bar))
                assert diff <= bar
        # the criterion's alpha spelled out
        assert np.array_equal(back2future.loss_summary(rec, like=like, pme_criterion="OSSIM", ssim_alpha=alpha)["loss"], s["loss"])
        assert not np.array_equal(back2future.loss_summary(rec, like=like)["loss"], s["loss"])


def test_argument_errors():
    table, ref = TL.tables(16, 16, 2, True, tame=True)
    rec16, rec24, rec32 = ops.table_loss(table, ref), ops.table_loss(table, ref, objective="finetune"), ops.table_loss(table, ref, objective="ssim")
    assert rec32.shape == (2, 2, 32)
    for rec in (rec16, rec24):
        for crit in ("OSSIM", "OSSIML1"):
            with pytest.raises(ValueError, match="32-word records of objective='ssim'"):
                back2future.loss_summary(rec, pme_criterion=crit)
    # a 32-word record with the default arguments is the 16-word summary
    a, b = back2future.loss_summary(rec32), back2future.loss_summary(rec16)
    assert np.array_equal(a["loss"], b["loss"]) and a["nonfinite"] == b["nonfinite"]
    for kw in ({"pme_criterion": "OBGCC"}, {"smooth_second_order": True}, {"objective": "Ours-Soft-ft-KITTI"}, {"ssim_alpha": 0.5},
               {"pme_criterion": "OSSIM", "ssim_alpha": 1.5}, {"pme_criterion": "SSIM"}):
        with pytest.raises(ValueError):
            back2future.loss_summary(rec32, **kw)
    with pytest.raises(ValueError):
        back2future.loss_summary(rec32[:, :, :28])
    for bad in ("clip", "", np.zeros((3, 2), F32), np.zeros((2,), F32), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            ops.table_loss(table, ref, objective="ssim", ssim_range=bad)
    with pytest.raises(ValueError):
        ops.table_loss(table, ref, objective="SSIM")


def test_the_host_entry_refuses_what_the_existing_one_refuses_and_a_bad_range():
    z = lambda c, h, w: np.zeros((1, c, h, w), np.float32)
    good = [z(2, 16, 16)] * 2 + [z(3, 16, 16)] * 2
    ref = z(3, 16, 16)
    out = np.full((1, 1, 32), 7, np.uint64)
    rng = np.array([0.0, 1.0], F32)

    def host(table, n_outs, n, H, W, past, scale=20.0, mode=SS.IMAGE, ranges=None):
        ptrs = (_lib.c_float_p * len(table))(*[_lib.fptr(t) if t is not None else None for t in table])
        return _lib.lib().b2f_table_loss_ssim_host(ptrs, n_outs, n, H, W, past, _lib.fptr(ref), scale, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), mode,
                                                   _lib.fptr(ranges) if ranges is not None else None)

    last = lambda: _lib.lib().b2f_last_error().decode()
    assert host(good, 0, 1, 16, 16, 0) != 0 and "n_outs" in last() and "b2f_table_loss_ssim_host" in last()
    assert host(good, 4, 1, 16, 16, 1) != 0                  # n_outs mismatch: four tensors are no Soft level
    assert host(good, 5, 1, 16, 16, 0) != 0 and "n_outs" in last()
    assert host(good[:3] + [None], 4, 1, 16, 16, 0) != 0 and "null" in last()
    assert host(good, 4, 1, 16, 16, 0, scale=0.0) != 0 and "flow_scale" in last()
    for mode in (-1, 3, 7):
        assert host(good, 4, 1, 16, 16, 0, mode=mode) != 0 and "range_mode" in last()
    assert host(good, 4, 1, 16, 16, 0, mode=SS.GIVEN) != 0 and "ranges" in last()
    assert (out == 7).all()                                  # nothing written by a refused call
    assert host(good, 4, 1, 16, 16, 0, mode=SS.GIVEN, ranges=rng) == 0 and out[0, 0, 0] == 256 and not out[0, 0, 26:].any()
    assert (out[0, 0, 22:24].astype(np.uint32).view(F32) == rng).all()
    assert _lib.lib().b2f_loss_ssim_weights(None) != 0 and "null" in last()
