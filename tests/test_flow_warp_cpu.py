"""CPU: motion compensation (the warped neighbours of models/pwc.lua:67-73 and the photometric record of
criterions/OBCCriterion.lua).  b2f_flow_warp_host against oracle.warping_unit, bit for bit, and against the numpy restatement of
include/b2f.h's record (tests/flow_warp_fields.py): all 14 words exactly equal, on fields with whole-pixel and zero flows, targets that
leave the image on every side or land exactly on its last column and row, NaN and Inf.  back2future.photo_summary against a
transcription of OBCCriterion:updateOutput.  The refusals need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from oracle import oracle
from tests import flow_warp_fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["b2f_flow_warp_host", "b2f_flow_warp_device", "b2f_op_flow_warp", "b2f_compute_flow_batch_warp",
         "b2f_compute_flow_sequence_warp", "b2f_multi_compute_flow_batch_warp", "b2f_multi_compute_flow_sequence_warp"]
ENUMS = {"B2F_PHOTO_INSIDE": 0, "B2F_PHOTO_OUTSIDE": 2, "B2F_PHOTO_CHARB_Q30": 4, "B2F_PHOTO_SQ_Q30": 6, "B2F_PHOTO_OCHARB_Q30": 8,
         "B2F_PHOTO_WEIGHT_Q30": 10, "B2F_PHOTO_NONFINITE": 12, "B2F_PHOTO_WORDS": 14}
SHAPES = [(1, 1), (37, 53), (64, 64), (150, 250)]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def test_the_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert re.search(r"B2F_API\s+int\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, lua), "lua cdef lacks " + n
        assert n + "(" in doc, "INTEGRATION.md does not quote " + n
    for e, v in ENUMS.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (e, v), src), e
    assert (back2future.PHOTO_INSIDE, back2future.PHOTO_OUTSIDE, back2future.PHOTO_CHARB_Q30, back2future.PHOTO_SQ_Q30,
            back2future.PHOTO_OCHARB_Q30, back2future.PHOTO_WEIGHT_Q30, back2future.PHOTO_NONFINITE, back2future.PHOTO_WORDS) == \
        (F.INSIDE, F.OUTSIDE, F.CHARB, F.SQ, F.OCHARB, F.WEIGHT, F.NONFINITE, F.WORDS)
    assert L.b2f_version() >= 1003
    # every comment of the new entries cites the reference's warp and criterion
    for n in NAMES:
        before = src[:src.index(n + "(")]
        comment = before[before.rindex("/*"):]
        assert ("BilinearSamplerBHWD.cu:88-104" in comment or "pwc.lua:67-73" in comment) and "OBCCriterion.lua:79-100" in comment, n


def _same_words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, want):
        b, k = np.argwhere(got != want)[0]
        raise AssertionError("%s: image %d word %d is %d, expected %d" % (what, b, k, got[b, k], want[b, k]))


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = got.reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        d = np.flatnonzero(a != b)
        raise AssertionError("%s: %d bytes differ, first at byte %d" % (what, d.size, d[0]))


@pytest.mark.parametrize("H,W", SHAPES)
def test_warped_floats_are_the_oracles_bit_for_bit(H, W):
    flow, ims, prob = F.fields(H, W, kind="unit")
    warped, photo = ops.flow_warp(flow, *ims, want_photo=False)
    assert photo is None and warped.dtype == np.float32 and warped.shape == (flow.shape[0], 2, 3, H, W)
    finite = np.isfinite(flow).all(axis=1)
    tame = np.where(finite[:, None], flow, np.float32(0))
    for d, (frame, k) in enumerate(((ims[0], -20.0), (ims[2], 20.0))):
        ref = oracle.warping_unit(frame, tame, k)
        nan = F.coordinates(flow, k)[2]
        m = np.broadcast_to(finite[:, None], ref.shape)
        assert m.any() or H * W == 1
        assert np.array_equal(warped[:, d][m].view(np.uint32), ref[m].view(np.uint32)), "direction %d differs from oracle.warping_unit" % d
        assert not warped[:, d][np.broadcast_to(nan[:, None], ref.shape)].view(np.uint32).any(), "a NaN coordinate gives +0"
    if H * W >= 64:
        assert (~finite).sum() >= 3 and F.coordinates(flow, 20.0)[2].any()


@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_host_entry_equals_the_definition(H, W, kind):
    flow, ims, prob = F.fields(H, W, kind=kind)
    for use_prob in (True, False):
        p = prob if use_prob else None
        w_want, nans, p_want = F.want(flow, *ims, occ_prob=p)
        warped, photo = ops.flow_warp(flow, *ims, occ_prob=p)
        what = "%dx%d %s occ_prob=%d" % (H, W, kind, use_prob)
        _same_bits(warped, F.quantise(w_want) if kind == "u8" else w_want, what + ": warped")
        _same_words(photo, p_want, what)
        if not use_prob:
            assert not photo[:, F.OCHARB:F.OCHARB + 2].any() and not photo[:, F.WEIGHT:F.WEIGHT + 2].any()
        # every pixel of every image is counted exactly once per direction
        for d in range(2):
            assert np.all(photo[:, F.INSIDE + d] + photo[:, F.OUTSIDE + d] + photo[:, F.NONFINITE + d] == H * W)
        # warped alone and photo alone are the same bytes and words
        only_w, none_p = ops.flow_warp(flow, *ims, occ_prob=p, want_photo=False)
        none_w, only_p = ops.flow_warp(flow, *ims, occ_prob=p, want_warped=False)
        assert none_p is None and none_w is None
        _same_bits(only_w, warped, what + ": warped alone")
        _same_words(only_p, photo, what + ": photo alone")
    if H * W >= 64:   # the fields reach every branch
        assert p_want[:, F.OUTSIDE:F.OUTSIDE + 2].all() and p_want[:, F.NONFINITE:F.NONFINITE + 2].all() and p_want[:, F.INSIDE:F.INSIDE + 2].all()
        # another scale is another record
        _same_words(ops.flow_warp(flow, *ims, occ_prob=prob, flow_scale=1.0, want_warped=False)[1], F.want(flow, *ims, occ_prob=prob, flow_scale=1.0)[2],
                    "flow_scale = 1")


def test_the_fields_land_exactly_on_the_border():
    """rows 1, 3 and 6 of the fields: targets exactly on the last column and row (future, past) and on column 0 / row 0: inside"""
    H, W = 37, 53
    flow = F.fields(H, W)[0]
    for row, k, col, line in ((1, 20.0, W - 1, H - 1), (3, -20.0, W - 1, H - 1), (6, 20.0, 0, 0)):
        xc, yc, nan, inside = F.coordinates(flow, k)
        ok = np.isfinite(flow[:, :, row]).all(axis=1) & (flow[:, 0, row] != 0)
        assert ok.sum() > W, "most whole-pixel values are exact in fp32"
        assert np.all(xc[:, row][ok] == col) and np.all(yc[:, row][ok] == line) and inside[:, row][ok].all()


@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_zero_flow_returns_the_neighbours(H, W, kind):
    _, ims, prob = F.fields(H, W, kind=kind)
    n = ims[0].shape[0]
    warped, photo = ops.flow_warp(np.zeros((n, 2, H, W), np.float32), *ims)
    _same_bits(warped[:, 0], ims[0], "past")
    _same_bits(warped[:, 1], ims[2], "future")
    assert np.all(photo[:, F.INSIDE:F.INSIDE + 2] == H * W) and not photo[:, F.OUTSIDE:F.OUTSIDE + 2].any() and not photo[:, F.NONFINITE:].any()


def test_the_quantisation_the_byte_outputs_are_held_against():
    """F.quantise, which test_host_entry_equals_the_definition applies to the oracle's floats, on hand-worked values of the rule
    v > 0 ? (v < 1 ? floorf(v * 255 + 0.5) : 255) : 0"""
    vals = np.array([0.0, -0.0, -1.0, 1.0, 2.0, np.nan, np.inf, -np.inf, 0.5, 0.25, 0.998], np.float32)
    assert F.quantise(vals).tolist() == [0, 0, 0, 255, 255, 0, 255, 0, 128, 64, 254]
    assert np.array_equal(F.quantise(np.arange(256, dtype=np.float32) / np.float32(255)), np.arange(256, dtype=np.uint8)), "k / 255 gives k back"


def test_photo_summary_is_the_criterion_of_the_reference():
    """pme against OBCCriterion:updateOutput (L1, penalty_out 1, sizeAverage) on finite fields: each pixel term rounds by at most 2^-31
    and a mean cannot lose more, so 1e-8 holds with room; bc, the PSNRs, the shares and pme_weighted against numpy."""
    for H, W in ((37, 53), (150, 250)):
        flow, ims, prob = F.fields(H, W, kind="unit")
        flow = np.where(np.isfinite(flow), flow, np.float32(0.25))
        prob = np.where(np.isfinite(prob), prob, np.float32(0.75))
        n = flow.shape[0]
        warped, photo = ops.flow_warp(flow, *ims, occ_prob=prob)
        s = back2future.photo_summary(photo)
        assert s["nonfinite"] == 0
        want = F.obcc_l1(flow, *ims, prob)
        print("%dx%d: pme %.12f, OBCCriterion %.12f, difference %.3g" % (H, W, s["pme"], want, s["pme"] - want))
        assert abs(s["pme"] - want) <= 1e-8
        ref = F.unit(ims[1]).astype(np.float64)
        inside = [F.coordinates(flow, k)[3] for k in (-20.0, 20.0)]
        delta = [warped[:, d].astype(np.float64) - ref for d in range(2)]
        charb = sum(np.sqrt(delta[d] ** 2 + 1e-6).sum(axis=1)[inside[d]].sum() for d in range(2))
        assert abs(s["bc"] - charb / (3.0 * (inside[0].sum() + inside[1].sum()))) <= 1e-8
        for d, key in enumerate(("psnr_past", "psnr_future")):
            mse = (delta[d] ** 2).sum(axis=1)[inside[d]].sum() / (3.0 * inside[d].sum())
            # d psnr = 10 / ln 10 * d mse / mse; d mse <= 2^-31 per pixel and mse >= 0.01 on random frames: 2e-7 at the most
            assert mse >= 0.01 and abs(s[key] - 10.0 * np.log10(1.0 / mse)) <= 1e-6
        assert s["inside_past"] == inside[0].sum() / float(n * H * W) and s["inside_future"] == inside[1].sum() / float(n * H * W)
        w = [prob[:, 1].astype(np.float64), prob[:, 0].astype(np.float64)]
        wsum = sum(w[d][inside[d]].sum() for d in range(2))
        wcharb = sum((np.sqrt(delta[d] ** 2 + 1e-6).sum(axis=1) * w[d])[inside[d]].sum() for d in range(2))
        assert abs(s["pme_weighted"] - wcharb / (3.0 * wsum)) <= 1e-8
        # one record and n records summarise alike; a single record is taken too
        assert back2future.photo_summary(photo[0])["pme"] == back2future.photo_summary(photo[:1])["pme"]
    with pytest.raises(ValueError):
        back2future.photo_summary(np.zeros((2, 13), np.uint64))
    with pytest.raises(ValueError):
        back2future.photo_summary(np.zeros((2, 14), np.int64))
    empty = back2future.photo_summary(np.zeros(14, np.uint64))
    assert np.isnan(empty["pme"]) and np.isnan(empty["psnr_past"]) and empty["nonfinite"] == 0


def test_photo_summary_counts_a_nonfinite_pixel_half():
    rec = np.zeros((1, 14), np.uint64)
    rec[0, F.INSIDE:F.INSIDE + 2] = (9, 10)
    rec[0, F.NONFINITE] = 1
    rec[0, F.OCHARB:F.OCHARB + 2] = (3 << 30, 6 << 30)
    s = back2future.photo_summary(rec)
    assert s["pme"] == 9.0 / (3 * 2 * 9.5) and s["nonfinite"] == 1 and s["inside_past"] == 0.9 and s["inside_future"] == 1.0


def test_refusals_before_any_gpu_work():
    H, W = 4, 5
    flow = np.zeros((1, 2, H, W), np.float32)
    im = np.zeros((1, 3, H, W), np.float32)
    for scale in (0.0, -20.0, float("nan"), float("inf")):
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            ops.flow_warp(flow, im, im, im, flow_scale=scale)
    with pytest.raises(_lib.B2FError, match="at least one of warped and photo"):
        ops.flow_warp(flow, im, im, im, want_warped=False, want_photo=False)
    L = _lib.lib()
    photo = np.zeros((1, 14), np.uint64)
    pp = photo.ctypes.data_as(C.POINTER(C.c_ulonglong))
    imp = C.c_void_p(im.ctypes.data)
    for kind in (back2future.IN_NORMALIZED, 3, -1):
        assert L.b2f_flow_warp_host(_lib.fptr(flow), None, 1, H, W, 20.0, kind, imp, imp, imp, None, pp) != 0
        assert "in_kind" in L.b2f_last_error().decode()
    assert L.b2f_flow_warp_host(_lib.fptr(flow), None, 1, H, W, 20.0, back2future.IN_UNIT, imp, None, imp, None, pp) != 0
    assert "null argument" in L.b2f_last_error().decode()
    assert L.b2f_flow_warp_host(_lib.fptr(flow), None, 0, H, W, 20.0, back2future.IN_UNIT, imp, imp, imp, None, pp) != 0
    assert "bad shape" in L.b2f_last_error().decode()
    # 2^28 pixels: refused from the shape alone, before any pointer is read
    assert L.b2f_flow_warp_host(_lib.fptr(flow), None, 1, 1 << 14, 1 << 14, 20.0, back2future.IN_UNIT, imp, imp, imp, None, pp) != 0
    assert "2^28" in L.b2f_last_error().decode()
    # the Python wrappers refuse malformed arrays themselves
    with pytest.raises(ValueError):
        ops.flow_warp(flow, im, im[:, :2], im)
    with pytest.raises(ValueError):
        ops.flow_warp(flow, im, im.astype(np.uint8), im)
    with pytest.raises(ValueError):
        ops.flow_warp(flow, im, im, im, occ_prob=np.zeros((1, 2, H, W + 1), np.float32))
