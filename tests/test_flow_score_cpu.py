"""CPU: flow scores against ground truth (the evaluation of test.lua:183-261 as integers).  b2f_flow_score_host against a plain numpy
restatement of include/b2f.h's definition (tests/flow_score_fields.py): all 22 words exactly equal, on fields that sit on the Fl
thresholds, saturate, carry NaN and Sintel's 1e9 marker under valid == 0, unlabelled occlusion bytes and rounding ties.
back2future.score_summary against a direct fp64 transcription of test.lua.  The refusals need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import flow_score_fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["b2f_flow_score_host", "b2f_flow_score_device", "b2f_op_flow_score", "b2f_compute_flow_batch_score",
         "b2f_compute_flow_sequence_score", "b2f_multi_compute_flow_batch_score", "b2f_multi_compute_flow_sequence_score"]
ENUMS = {"B2F_SCORE_PIXELS": 0, "B2F_SCORE_EPE_Q20": 4, "B2F_SCORE_OUTLIERS": 8, "B2F_SCORE_OCC": 12, "B2F_SCORE_NONFINITE": 21,
         "B2F_SCORE_WORDS": 22}
SHAPES = [(1, 1), (37, 53), (64, 64)]


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
        assert e in lua and e in doc, e
    assert (back2future.SCORE_PIXELS, back2future.SCORE_EPE_Q20, back2future.SCORE_OUTLIERS, back2future.SCORE_OCC,
            back2future.SCORE_NONFINITE, back2future.SCORE_WORDS) == (0, 4, 8, 12, 21, 22)
    assert L.b2f_version() >= 1002
    # every comment of the new entries cites the reference's evaluation
    for n in NAMES:
        before = src[:src.index(n + "(")]
        comment = before[before.rindex("/*"):]
        assert "test.lua:183-261" in comment and "L2Criterion.lua:36-38" in comment, n


def _same_words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, want):
        b, k = np.argwhere(got != want)[0]
        raise AssertionError("%s: image %d word %d is %d, expected %d" % (what, b, k, got[b, k], want[b, k]))


@pytest.mark.parametrize("H,W", SHAPES)
def test_host_entry_equals_the_numpy_restatement(H, W):
    fl = F.fields(H, W)
    flow, gt = fl[0], fl[1]
    for combo in F.combos():
        kw = F.pick(fl, *combo)
        got = ops.flow_score(flow, gt, **kw)
        want = F.numpy_scores(flow, gt, **kw)
        _same_words(got, want, "%dx%d valid=%d gt_occ=%d occ_prob=%d" % ((H, W) + combo))
        if not (combo[1] and combo[2]):
            assert not got[:, F.OCC:F.OCC + 9].any(), "the matrix needs both gt_occ and occ_prob"
        if not combo[1]:
            assert not got[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].any(), "without gt_occ everything is bucket 3"
    # another scale is another score
    _same_words(ops.flow_score(flow, gt, flow_scale=1.0, **F.pick(fl, True, True, True)),
                F.numpy_scores(flow, gt, flow_scale=1.0, **F.pick(fl, True, True, True)), "flow_scale = 1")


def _one(px, use_valid=True):
    """the record of one special pixel"""
    a = lambda v, dt: np.array(v, dt).reshape(1, -1, 1, 1)
    return ops.flow_score(a(px[0:2], np.float32), a(px[2:4], np.float32), occ_prob=a(px[6:8], np.float32),
                          valid=np.array(px[4], np.uint8).reshape(1, 1, 1) if use_valid else None,
                          gt_occ=np.array(px[5], np.uint8).reshape(1, 1, 1))[0]


def _record(**words):
    r = np.zeros(F.WORDS, np.uint64)
    for k, v in words.items():
        r[int(k[1:])] = v
    return r


def test_the_special_pixels_score_as_the_definition_says():
    """Each of the pixels the fields carry, alone, against the words worked out by hand (wK = word K of the record)."""
    q = lambda err: int(err * 1048576.0 + 0.5)
    sat = 65536 << 20
    just_above_3 = 12.5 - float(F.SPECIAL[2][2])     # exact in fp64
    assert 3.0 < just_above_3 < 3.000001
    expect = [
        _record(w1=1, w5=q(3.0), w16=1),                          # err == 3: no outlier; 0.5 rounds away from zero: cell [1][1]
        _record(w1=1, w5=q(3.0), w17=1),                          # err == 3 again; 1.5 -> class 2: cell [1][2]
        _record(w0=1, w4=q(just_above_3), w8=1, w13=1),           # err > 3 > 0.05 |gt|: outlier; cell [0][1]
        _record(w2=1, w6=q(102.5 - float(F.SPECIAL[3][2])), w20=1),   # 3 < err < 0.05 |gt|: no outlier; cell [2][2]
        _record(w1=1, w5=q(5.0), w17=1),                          # err == 0.05 |gt|: no outlier; 6 clamps to class 2
        _record(w1=1, w5=q(float(F.SPECIAL[5][0]) * 20.0 - 100.0), w9=1, w15=1),   # err > 0.05 |gt| > 3: outlier; -4 clamps to class 0
        _record(w2=1, w6=sat, w10=1, w19=1),                      # saturated; |gt| = 0: outlier; (1 - .5) + .5 = 1: cell [2][1]
        _record(w3=1, w7=sat, w11=1),                             # label 3: bucket 3, no cell
        _record(w15=1),                                           # invalid: only the matrix sees it, 0.15 -> class 0: cell [1][0]
        _record(w14=1),                                           # invalid; 1.85 -> class 2: cell [0][2]
        _record(),                                                # invalid and unlabelled: nothing
        _record(w21=1, w16=1),                                    # NaN under valid: nonfinite only; 0.9 -> class 1: cell [1][1]
        _record(w21=1),                                           # NaN, mask byte 7, label 3
        _record(w21=1, w19=1),                                    # inf - inf; cell [2][1]
        _record(w3=1),                                            # label 255: bucket 3; the error is 2e-8 px, 0 in Q20
        _record(w3=1),                                            # label 3: the same
    ]
    assert len(expect) == len(F.SPECIAL)
    for j, want in enumerate(expect):
        got = _one(F.SPECIAL[j])
        assert np.array_equal(got, want), (j, F.SPECIAL[j], got.tolist(), want.tolist())
    # with no mask the 1e9 marker counts, saturated
    assert _one(F.SPECIAL[8], use_valid=False)[F.EPE_Q20 + 1] == sat


def test_invalid_pixels_change_nothing():
    """Whatever stands under valid == 0 -- Sintel's 1e9, NaN, inf, in the flow or in the ground truth -- the flow words are the same."""
    flow, gt, prob, valid, occ = F.fields(37, 53)
    base = ops.flow_score(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ)
    off = valid == 0
    assert off.any()
    for junk in (1e9, np.nan, np.inf, -np.inf):
        g2, f2 = gt.copy(), flow.copy()
        g2[:, 0][off] = junk
        g2[:, 1][off] = junk
        f2[:, 1][off] = junk
        _same_words(ops.flow_score(f2, g2, occ_prob=prob, valid=valid, gt_occ=occ), base, "junk %r under valid == 0" % junk)


def test_lua_reference(H=48, W=80, n=3):
    """score_summary against test.lua:183-261 transcribed to fp64 numpy: raw units first, then times flownet_factor (:190-192), one
    occlusion channel (3 classes) for the EPE split and for the accuracies here.  The records round every error to 2^-20 px, i.e. by
    at most 2^-21 px per pixel, so a mean of errors is within 2^-21 < 1e-6 px of the unrounded one; ratios of counts are exact."""
    r = np.random.default_rng(11)
    factor = 20.0
    flow = r.normal(0, 0.3, (n, 2, H, W)).astype(np.float32)
    gt = (flow * np.float32(factor) + r.normal(0, 3, (n, 2, H, W))).astype(np.float32)
    prob = r.random((n, 2, H, W), dtype=np.float32)
    valid = (r.random((n, H, W)) < 0.8).astype(np.uint8)
    occ = r.choice(np.array([0, 1, 1, 2], np.uint8), (n, H, W))
    got = back2future.score_summary(ops.flow_score(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ, flow_scale=factor))
    # criterion:forward(outputs[1], {labels[1..2], masks}) on labels in raw units (L2Criterion.lua:36-38)
    labels, masks = gt.astype(np.float64) / factor, valid.astype(np.float64)
    epe_map = np.sqrt(((flow.astype(np.float64) - labels) ** 2).sum(1)) * masks
    want = {"epe": epe_map.sum() / masks.sum() * factor}
    lbl_occ = occ.astype(np.float64) / 2
    o = lbl_occ != 0.5                                                            # :198-208
    want["epe_noc"] = np.where(o, 0, epe_map).sum() / ((1 - o) * masks).sum() * factor
    v = lbl_occ == 0.5                                                            # :212-222
    want["epe_occ"] = np.where(v, 0, epe_map).sum() / ((1 - v) * masks).sum() * factor
    est = F._round_half_away((np.float32(1) - prob[:, 0]) + prob[:, 1]).astype(np.float64) * 0.5   # :236
    hit = lbl_occ == est
    want["oacc"] = hit.sum() / lbl_occ.size                                       # :241-242
    for name, cls in (("occ_acc_bwd", 0.0), ("occ_acc_vis", 0.5), ("occ_acc_fwd", 1.0)):
        want[name] = hit[lbl_occ == cls].sum() / (lbl_occ == cls).sum()           # :244-259
    for k in ("epe", "epe_noc", "epe_occ"):
        print("%s: %.9f, test.lua %.9f" % (k, got[k], want[k]), flush=True)
        assert abs(got[k] - want[k]) <= 1e-6, k
    for k in ("oacc", "occ_acc_bwd", "occ_acc_vis", "occ_acc_fwd"):
        assert got[k] == want[k], (k, got[k], want[k])
    words = F.numpy_scores(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ, flow_scale=factor)
    assert got["fl"] == int(words[:, 8:12].sum()) / int(valid.sum())   # test.lua has no Fl: KITTI's rule on the same errors
    assert got["pixels"] == int(valid.sum()) and got["nonfinite"] == 0


def test_score_summary_sums_images_and_marks_empty_ratios():
    flow, gt, prob, valid, occ = F.fields(37, 53)
    s = ops.flow_score(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ)
    every = back2future.score_summary(s)
    t = s.sum(0, dtype=np.uint64)
    assert every == back2future.score_summary(t)
    assert every["pixels"] == int(t[0:4].sum()) and every["nonfinite"] == int(t[21]) > 0
    assert every["fl"] == int(t[8:12].sum()) / int(t[0:4].sum())
    assert every["epe"] == int(t[4:8].sum()) / 2.0 ** 20 / int(t[0:4].sum())
    assert every["epe_noc"] == int(t[5]) / 2.0 ** 20 / int(t[1])
    assert every["epe_occ"] == (int(t[4]) + int(t[6])) / 2.0 ** 20 / (int(t[0]) + int(t[2]))
    assert every["oacc"] == (int(t[12]) + int(t[16]) + int(t[20])) / int(t[12:21].sum())
    assert every["occ_acc_fwd"] == int(t[20]) / int(t[18:21].sum())
    none = back2future.score_summary(ops.flow_score(flow, gt))
    for k in ("epe_noc", "epe_occ", "oacc", "occ_acc_bwd", "occ_acc_vis", "occ_acc_fwd"):
        assert np.isnan(none[k]), k
    assert none["epe"] > 0 and none["pixels"] == 3 * 37 * 53 - none["nonfinite"]
    empty = back2future.score_summary(np.zeros(22, np.uint64))
    assert all(np.isnan(empty[k]) for k in ("epe", "fl")) and empty["pixels"] == 0
    with pytest.raises(ValueError):
        back2future.score_summary(np.zeros(22, np.int64))
    with pytest.raises(ValueError):
        back2future.score_summary(np.zeros((2, 21), np.uint64))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
H, W = 64, 64
FRAMES = np.zeros((3, 3, H, W), np.float32)
FLOW = np.zeros((1, 2, H, W), np.float32)
GT = np.zeros((1, 2, H, W), np.float32)
BYTES = np.zeros((1, H, W), np.uint8)
SCORES = np.zeros((1, 22), np.uint64)
M1, M2 = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8)
_vp = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
_sp = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong)) if a is not None else None
_fp = lambda a: _lib.fptr(a) if a is not None else None


def _call(name, count=None, h=H, w=W, scale=20.0, flow=FLOW, gt=GT, scores=SCORES, offset=0):
    """One call of `name` with a null context and every other argument valid"""
    L = _lib.lib()
    if name == "b2f_flow_score_host":
        return L.b2f_flow_score_host(_fp(flow), None, 1 if count is None else count, h, w, scale, _fp(gt), _up(BYTES), _up(BYTES), _sp(scores))
    if name == "b2f_op_flow_score":
        return L.b2f_op_flow_score(None, _fp(flow), None, 1 if count is None else count, h, w, scale, _fp(gt), _up(BYTES), _up(BYTES), _sp(scores))
    if name == "b2f_flow_score_device":
        return L.b2f_flow_score_device(None, _vp(flow, offset), None, 1 if count is None else count, h, w, scale, _vp(gt), _vp(BYTES), _vp(BYTES),
                                       _vp(scores), None)
    seq = "sequence" in name
    count = (3 if seq else 1) if count is None else count
    ins = [_vp(FRAMES)] if seq else [_vp(FRAMES)] * 3
    return getattr(L, name)(None, count, back2future.IN_UNIT, *ins, h, w, scale, _fp(gt), _up(BYTES), _up(BYTES), _sp(scores), _fp(flow),
                            _up(M1), _up(M2))


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_fail_with_a_message_before_any_hip_call(name):
    compute = "compute_flow" in name
    cases = [
        (dict(scale=0.0), "flow_scale"),
        (dict(scale=-20.0), "flow_scale"),
        (dict(scale=float("nan")), "flow_scale"),
        (dict(scale=float("inf")), "flow_scale"),
        (dict(h=0), "bad shape"),
        (dict(w=-5), "bad shape"),
        (dict(h=16384, w=16384), "2^28 pixels"),
        (dict(gt=None), "null argument"),
        (dict(scores=None), "null argument"),
    ]
    if "sequence" in name:
        cases += [(dict(count=2), "T >= 3"), (dict(count=0), "T >= 3")]
    else:
        cases.append((dict(count=0), "bad shape"))
    if not compute:
        cases.append((dict(flow=None), "null argument"))   # the computeFlow forms may leave the flow out
    if name != "b2f_flow_score_host":
        cases.append((dict(), "null context"))
    for kw, msg in cases:
        rc = _call(name, **kw)
        assert rc != 0, (name, kw)
        err = _lib.lib().b2f_last_error().decode()
        assert name in err and msg in err, (name, kw, err)
    if compute:   # without the flow the request is still complete: the first complaint is the context
        assert _call(name, flow=None) != 0
        assert "null context" in _lib.lib().b2f_last_error().decode()
    if name == "b2f_flow_score_host":   # the largest image that is not refused for its size would need 2 GB: the bound itself
        assert _call(name, h=16384, w=16383, flow=None) != 0
        assert "null argument" in _lib.lib().b2f_last_error().decode()


def test_the_device_entry_refuses_misaligned_pointers():
    assert _call("b2f_flow_score_device", offset=4) != 0
    err = _lib.lib().b2f_last_error().decode()
    assert "b2f_flow_score_device" in err and "16-byte aligned" in err, err
    assert _call("b2f_flow_score_device", offset=16) != 0
    assert "null context" in _lib.lib().b2f_last_error().decode()


class _NoLib(back2future.Model):
    def __init__(self):
        self._h = None


class _NoLibMulti(back2future.MultiModel):
    def __init__(self):
        self._h = None


@pytest.fixture
def no_library(monkeypatch):
    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_call)


@pytest.mark.parametrize("cls", [_NoLib, _NoLibMulti])
def test_wrappers_validate_before_calling_the_library(cls, no_library):
    m = cls()
    V = np.zeros((4, 3, 64, 64), np.float32)
    gt = np.zeros((2, 2, 64, 64), np.float32)
    with pytest.raises(ValueError, match="gt_flow"):
        m.computeFlowSequenceScore(V, gt[:1])
    with pytest.raises(ValueError, match="valid"):
        m.computeFlowSequenceScore(V, gt, valid=np.zeros((2, 64, 64), np.float32))
    with pytest.raises(ValueError, match="gt_occ"):
        m.computeFlowBatchScore(V[:2], V[:2], V[:2], gt, gt_occ=np.zeros((2, 64, 63), np.uint8))
    with pytest.raises(ValueError, match="out"):
        m.computeFlowBatchScore(V[:2], V[:2], V[:2], gt, out=np.zeros((2, 22), np.int64))
    with pytest.raises(ValueError, match="out must be"):
        m.computeFlowSequenceScore(V, gt, want_flow=True, out=(np.zeros((2, 22), np.uint64),))
    with pytest.raises(ValueError, match="expected three"):
        m.computeFlowBatchScore(V[:2], V[:2], V[:3], gt)


def test_flow_score_validates_before_calling_the_library(no_library):
    f = np.zeros((2, 2, 8, 8), np.float32)
    with pytest.raises(ValueError, match="n x 2 x H x W"):
        ops.flow_score(f[0], f[0])
    with pytest.raises(ValueError, match="gt_flow"):
        ops.flow_score(f, f[:, :, :4])
    with pytest.raises(ValueError, match="occ_prob"):
        ops.flow_score(f, f, occ_prob=f[:1])
    with pytest.raises(ValueError, match="bad shape"):
        _NoLib().flowScoreDevice(16, 0, 8, 8, 16, 16)
