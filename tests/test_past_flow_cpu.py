"""CPU: the Soft models' past flow at the ABI and motion compensation with it (models/pwc.lua:425-432,
criterions/OBCCriterion.lua:80-81).  Every new entry is declared, exported, bound and quoted; b2f_flow_warp_past_host against
oracle.warping_unit of the past flow bit for bit, against b2f_flow_warp_host wherever the past flow plays no part, and against the numpy
restatement of include/b2f.h's record with the past coordinate: all 14 words equal.  back2future.photo_summary against a
transcription of OBCCriterion:updateOutput with past_flow = true.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from oracle import oracle
from tests import flow_warp_fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> arguments of the C prototype
ENTRIES = {
    "b2f_forward_device_past": 11, "b2f_forward_sequence_device_past": 11,
    "b2f_compute_flow_batch_past": 13, "b2f_compute_flow_sequence_past": 11,
    "b2f_compute_flow_device_past": 14, "b2f_compute_flow_sequence_device_past": 12,
    "b2f_multi_compute_flow_batch_past": 13, "b2f_multi_compute_flow_sequence_past": 11,
    "b2f_flow_warp_past_host": 13, "b2f_flow_warp_past_device": 15, "b2f_op_flow_warp_past": 14,
    "b2f_compute_flow_batch_warp_past": 16, "b2f_compute_flow_sequence_warp_past": 14,
    "b2f_multi_compute_flow_batch_warp_past": 16, "b2f_multi_compute_flow_sequence_warp_past": 14,
}
# the entry without the past flow: the new one has its arguments plus one
TWINS = {
    "b2f_forward_device_past": "b2f_forward_device", "b2f_forward_sequence_device_past": "b2f_forward_sequence_device",
    "b2f_compute_flow_batch_past": "b2f_compute_flow_batch_f32", "b2f_compute_flow_sequence_past": "b2f_compute_flow_sequence_f32",
    "b2f_compute_flow_device_past": "b2f_compute_flow_device", "b2f_compute_flow_sequence_device_past": "b2f_compute_flow_sequence_device",
    "b2f_multi_compute_flow_batch_past": "b2f_multi_compute_flow_batch_f32",
    "b2f_multi_compute_flow_sequence_past": "b2f_multi_compute_flow_sequence_f32",
    "b2f_flow_warp_past_host": "b2f_flow_warp_host", "b2f_flow_warp_past_device": "b2f_flow_warp_device",
    "b2f_op_flow_warp_past": "b2f_op_flow_warp", "b2f_compute_flow_batch_warp_past": "b2f_compute_flow_batch_warp",
    "b2f_compute_flow_sequence_warp_past": "b2f_compute_flow_sequence_warp",
    "b2f_multi_compute_flow_batch_warp_past": "b2f_multi_compute_flow_batch_warp",
    "b2f_multi_compute_flow_sequence_warp_past": "b2f_multi_compute_flow_sequence_warp",
}
SHAPES = [(1, 1), (5, 7), (33, 61), (64, 64)]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def _arguments(src, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_the_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "b2f.h")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.SO_PATH)
    for n, argc in ENTRIES.items():
        assert re.search(r"B2F_API\s+int\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
        args = _arguments(src, n)
        assert len(args) == argc == len(_lib.SIGNATURES[n][1]), (n, len(args), len(_lib.SIGNATURES[n][1]))
        assert len(_arguments(lua, n)) == argc, "lua cdef: " + n
        assert n + "(" in doc, "INTEGRATION.md does not quote " + n
        # the twin's arguments in the twin's order, with the past flow right after the flow
        twin = _arguments(src, TWINS[n])
        at = [i for i, a in enumerate(args) if a.endswith("past_flow")]
        assert len(at) == 1 and "float *" in args[at[0]], (n, args)
        assert args[at[0] - 1].endswith("flow") and not args[at[0] - 1].endswith("past_flow"), (n, args)
        assert args[:at[0]] + args[at[0] + 1:] == twin, (n, args, twin)
    assert L.b2f_version() >= 1005
    # the sign is documented where the entries are
    assert "x - past_flow * flow_scale" in src and "past_flow == flow" in src
    assert "is not a `computeFlow` output" not in open(os.path.join(ROOT, "DESIGN.md")).read()
    for cls in (back2future.Model, back2future.MultiModel):
        for meth in ("computeFlowBatchPast", "computeFlowSequencePast"):
            assert callable(getattr(cls, meth)), meth
    for meth in ("computeFlowDevicePast", "computeFlowSequenceDevicePast"):
        assert callable(getattr(back2future.Model, meth)), meth


def _same_words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, want):
        b, k = np.argwhere(got != want)[0]
        raise AssertionError("%s: image %d word %d is %d, expected %d" % (what, b, k, got[b, k], want[b, k]))


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        d = np.flatnonzero(a != b)
        raise AssertionError("%s: %d bytes differ, first at byte %d" % (what, d.size, d[0]))


def past_field(H, W, n=3):
    """A past flow for F.fields(H, W): the same kind of field from another seed -- its own whole-pixel rows, targets that leave the
    image, exact hits of the last column and row for k = -20 (row 3) and of column 0 / row 0 for k = +20 (row 6, which the past frame
    leaves), NaN and +-Inf -- with further specials where the future flow is finite, so that the two differ in where they are
    non-finite.  A tiny image's field does not depend on the seed (zero, NaN and Inf from image to image): there the past flow is the
    field of images 9, 10, ...: (0.01, 0.01), (0, 0), (NaN, 0) against the flow's (0, 0), (NaN, 0), (Inf, NaN)."""
    if H * W < 64:
        return F.fields(H, W, n=n + 9, seed=1)[0][9:].copy()
    past = F.fields(H, W, n=n, seed=1)[0].copy()
    if H * W >= 64:
        specials = [np.inf, np.nan, -np.inf]
        for b in range(n):
            for j in range(6):
                i = (j * 41 + 3 * b + 17) % (H * W)
                past[b, (j + 1) % 2, i // W, i % W] = specials[j % 3]
    return past


def want_past(flow, past, im1, im2, im3, occ_prob=None, flow_scale=F.SCALE):
    """include/b2f.h's definition with the past coordinate, restated through tests/flow_warp_fields.want: direction 0 (planes and
    words) is what the definition gives when the flow is the past flow, direction 1 what it gives for the flow itself."""
    w_p, nan_p, ph_p = F.want(past, im1, im2, im3, occ_prob=occ_prob, flow_scale=flow_scale)
    w_f, nan_f, ph_f = F.want(flow, im1, im2, im3, occ_prob=occ_prob, flow_scale=flow_scale)
    warped = np.stack([w_p[:, 0], w_f[:, 1]], axis=1)
    photo = ph_f.copy()
    photo[:, 0::2] = ph_p[:, 0::2]   # word = base + d: the even words are direction 0
    return warped, photo


@pytest.mark.parametrize("H,W", SHAPES)
def test_past_planes_are_the_oracles_warp_of_the_past_flow(H, W):
    flow, ims, prob = F.fields(H, W, kind="unit")
    past = past_field(H, W)
    warped, photo = ops.flow_warp(flow, *ims, want_photo=False, own_past_flow=True, past_flow=past)
    plain = ops.flow_warp(flow, *ims, want_photo=False)[0]
    assert photo is None and warped.dtype == np.float32 and warped.shape == (flow.shape[0], 2, 3, H, W)
    finite = np.isfinite(past).all(axis=1)
    tame = np.where(finite[:, None], past, np.float32(0))
    ref = oracle.warping_unit(ims[0], tame, -F.SCALE)
    m = np.broadcast_to(finite[:, None], ref.shape)
    assert m.any() or H * W == 1
    assert np.array_equal(warped[:, 0][m].view(np.uint32), ref[m].view(np.uint32)), "d = 0 differs from oracle.warping_unit(im1, past_flow, -scale)"
    nan = F.coordinates(past, -F.SCALE)[2]
    assert not warped[:, 0][np.broadcast_to(nan[:, None], ref.shape)].view(np.uint32).any(), "a NaN coordinate gives +0"
    _same_bits(warped[:, 1], plain[:, 1], "d = 1 planes are b2f_flow_warp_host's")
    assert not np.array_equal(past, flow, equal_nan=True)
    if H * W >= 64:
        assert not np.array_equal(warped[:, 0], plain[:, 0]), "the past flow moved nothing"


@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_host_entry_equals_the_definition_with_the_past_coordinate(H, W, kind):
    flow, ims, prob = F.fields(H, W, kind=kind)
    past = past_field(H, W)
    for use_prob in (True, False):
        p = prob if use_prob else None
        what = "%dx%d %s occ_prob=%d" % (H, W, kind, use_prob)
        w_want, p_want = want_past(flow, past, *ims, occ_prob=p)
        warped, photo = ops.flow_warp(flow, *ims, occ_prob=p, own_past_flow=True, past_flow=past)
        _same_bits(warped, F.quantise(w_want) if kind == "u8" else w_want, what + ": warped")
        _same_words(photo, p_want, what)
        for d in range(2):   # every pixel of every image is counted exactly once per direction
            assert np.all(photo[:, F.INSIDE + d] + photo[:, F.OUTSIDE + d] + photo[:, F.NONFINITE + d] == H * W)
        # direction 1 is the plain entry's, planes and words
        w_plain, p_plain = ops.flow_warp(flow, *ims, occ_prob=p)
        _same_bits(warped[:, 1], w_plain[:, 1], what + ": d = 1 planes")
        _same_words(np.ascontiguousarray(photo[:, 1::2]), np.ascontiguousarray(p_plain[:, 1::2]), what + ": d = 1 words")
        # the flow as its own past flow: the plain entry's every byte and word
        w_same, p_same = ops.flow_warp(flow, *ims, occ_prob=p, own_past_flow=True, past_flow=flow)
        _same_bits(w_same, w_plain, what + ": past_flow is flow, warped")
        _same_words(p_same, p_plain, what + ": past_flow is flow")
        # warped alone and photo alone are the same bytes and words
        only_w, none_p = ops.flow_warp(flow, *ims, occ_prob=p, want_photo=False, own_past_flow=True, past_flow=past)
        none_w, only_p = ops.flow_warp(flow, *ims, occ_prob=p, want_warped=False, own_past_flow=True, past_flow=past)
        assert none_p is None and none_w is None
        _same_bits(only_w, warped, what + ": warped alone")
        _same_words(only_p, photo, what + ": photo alone")
    if H * W >= 64:   # the past field reaches every branch of direction 0, and not where the flow does
        assert p_want[:, F.OUTSIDE].all() and p_want[:, F.NONFINITE].all() and p_want[:, F.INSIDE].all()
        assert not np.array_equal(p_want[:, 0::2], F.want(flow, *ims, occ_prob=prob)[2][:, 0::2])
        _same_words(ops.flow_warp(flow, *ims, occ_prob=prob, flow_scale=1.0, want_warped=False, own_past_flow=True, past_flow=past)[1],
                    want_past(flow, past, *ims, occ_prob=prob, flow_scale=1.0)[1], "flow_scale = 1")


def test_the_past_field_lands_exactly_on_the_border():
    """row 3 of the past field: targets of k = -20 exactly on the last column and row: inside"""
    H, W = 33, 61
    past = past_field(H, W)
    xc, yc, nan, inside = F.coordinates(past, -20.0)
    ok = np.isfinite(past[:, :, 3]).all(axis=1) & (past[:, 0, 3] != 0)
    assert ok.sum() > W, "most whole-pixel values are exact in fp32"
    assert np.all(xc[:, 3][ok] == W - 1) and np.all(yc[:, 3][ok] == H - 1) and inside[:, 3][ok].all()


def obcc_l1_past(flow, past, im1, im2, im3, occ_prob, flow_scale=F.SCALE):
    """criterions/OBCCriterion.lua:36-119 with past_flow = true (:80-81: the past frame's target is coord + (f - ref - 1) * input[2] *
    pwc_flow_scaling, input[2] the past flow), otherwise as tests/flow_warp_fields.obcc_l1: L1 penalty with eps = 0.001 * 0.001,
    penalty_out = 1, sizeAverage, F = 3, on the warps of oracle.warping_unit (the past frame by the past flow, pwc.lua:425-432).
    Coordinates 1-based fp32, sums fp64."""
    n, _, H, W = flow.shape
    F32 = np.float32
    warps = (oracle.warping_unit(F.unit(im1), past, float(F32(-flow_scale))), oracle.warping_unit(F.unit(im3), flow, float(F32(flow_scale))))
    target = F.unit(im2).astype(np.float64)
    coord_x = np.arange(1, W + 1, dtype=F32)[None, None, :]
    coord_y = np.arange(1, H + 1, dtype=F32)[None, :, None]
    eps = 0.001 * 0.001
    acc = np.zeros((n, H, W), np.float64)
    for f in (1, 2):
        buffer = warps[f - 1].astype(np.float64) - target
        tmp = np.power(buffer * buffer + eps, 0.5).sum(axis=1)
        if f <= 1.0:   # ref = 0.5 * (F - 1) = 1
            tx = coord_x + (F32(f - 1 - 1) * past[:, 0]) * F32(flow_scale)
            ty = coord_y + (F32(f - 1 - 1) * past[:, 1]) * F32(flow_scale)
            tmp = tmp * occ_prob[:, 1].astype(np.float64)
        else:
            tx = coord_x + (F32(f - 1) * flow[:, 0]) * F32(flow_scale)
            ty = coord_y + (F32(f - 1) * flow[:, 1]) * F32(flow_scale)
            tmp = tmp * occ_prob[:, 0].astype(np.float64)
        mask = ((tx >= 1) & (ty >= 1) & (tx <= W) & (ty <= H)).astype(np.float64)
        acc += tmp * mask + (1.0 - mask) * 1.0
    norm = 3.0 / (n * 3.0 * H * W)
    return norm * (acc.sum() / (3.0 * 2.0))


def test_photo_summary_is_the_criterion_of_the_reference_with_past_flow():
    """pme against OBCCriterion:updateOutput with past_flow = true on finite fields, within the 1e-8 of
    tests/test_flow_warp_cpu.py::test_photo_summary_is_the_criterion_of_the_reference (a pixel term rounds by at most 2^-31)."""
    for H, W in ((33, 61), (64, 64)):
        flow, ims, prob = F.fields(H, W, kind="unit")
        past = past_field(H, W)
        flow = np.where(np.isfinite(flow), flow, np.float32(0.25))
        past = np.where(np.isfinite(past), past, np.float32(-0.35))
        prob = np.where(np.isfinite(prob), prob, np.float32(0.75))
        photo = ops.flow_warp(flow, *ims, occ_prob=prob, want_warped=False, own_past_flow=True, past_flow=past)[1]
        s = back2future.photo_summary(photo)
        assert s["nonfinite"] == 0
        want = obcc_l1_past(flow, past, *ims, prob)
        plain = F.obcc_l1(flow, *ims, prob)
        print("%dx%d: pme %.12f, OBCCriterion(past_flow) %.12f, difference %.3g; without the past flow %.12f" %
              (H, W, s["pme"], want, s["pme"] - want, plain))
        assert abs(s["pme"] - want) <= 1e-8
        assert abs(want - plain) > 1e-4, "the fields do not tell the two criteria apart"


def test_refusals_before_any_gpu_work():
    H, W = 4, 5
    flow = np.zeros((1, 2, H, W), np.float32)
    im = np.zeros((1, 3, H, W), np.float32)
    with pytest.raises(ValueError, match="own_past_flow"):
        ops.flow_warp(flow, im, im, im, own_past_flow=True)
    with pytest.raises(ValueError, match="own_past_flow"):
        ops.flow_warp(flow, im, im, im, past_flow=flow)
    with pytest.raises(ValueError, match="past_flow"):
        ops.flow_warp(flow, im, im, im, own_past_flow=True, past_flow=np.zeros((1, 2, H, W + 1), np.float32))
    with pytest.raises(_lib.B2FError, match="flow_scale"):
        ops.flow_warp(flow, im, im, im, flow_scale=0.0, own_past_flow=True, past_flow=flow)
    L = _lib.lib()
    photo = np.zeros((1, 14), np.uint64)
    pp = photo.ctypes.data_as(C.POINTER(C.c_ulonglong))
    imp = C.c_void_p(im.ctypes.data)
    assert L.b2f_flow_warp_past_host(_lib.fptr(flow), None, None, 1, H, W, 20.0, back2future.IN_UNIT, imp, imp, imp, None, pp) != 0
    assert "past_flow" in L.b2f_last_error().decode()
    assert L.b2f_flow_warp_past_host(_lib.fptr(flow), _lib.fptr(flow), None, 1, H, W, 20.0, back2future.IN_UNIT, imp, imp, imp, None, None) != 0
    assert "at least one of warped and photo" in L.b2f_last_error().decode()
