"""GPU: flow scores against ground truth as an output stage.  b2f_op_flow_score against the host entry b2f_flow_score_host (which
tests/test_flow_score_cpu.py holds against a numpy restatement): all 22 words of every record equal -- the sums are integers, so no
tolerance is involved.  Everything above the kernel is defined from it: b2f_flow_score_device and the computeFlow*Score entries give
ops.flow_score of the float32 flow and occ_prob the existing f32 entries return, however the request is cut."""
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, flow_io, ops, weights as W
from tests import flow_score_fields as F
from tests import trained_like as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MEAN = np.array([0.485, 0.456, 0.406] * 3, np.float32).reshape(1, 9, 1, 1)
STD = np.array([0.229, 0.224, 0.225] * 3, np.float32).reshape(1, 9, 1, 1)


def _clip(seed, T, H0, W0, kind):
    r = np.random.default_rng(seed)
    if kind == "unit":
        return r.random((T, 3, H0, W0), dtype=np.float32)
    return r.integers(0, 256, (T, 3, H0, W0), dtype=np.uint8)


def _triplets(V):
    return [np.ascontiguousarray(a) for a in (V[:-2], V[1:-1], V[2:])]


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def soft():
    m = back2future.Model("random:soft:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def trained():
    """A Soft model with weights like trained ones (tests/trained_like.py), so that the flows span many pixels (x 20: raw units)"""
    V = _clip(1, 3, 128, 192, "unit")
    x = np.concatenate(_triplets(V), axis=1)
    params = TL.calibrate(W.random_init(7, True, 1.0), ((x + (-MEAN)) / STD).astype(np.float32), True)
    m = back2future.Model("random:soft:1:1.0")
    m.set_weights(params)
    yield m
    m.close()


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    x, y = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
    if not np.array_equal(x, y):
        d = np.flatnonzero(x != y)
        raise AssertionError("%s: %d bytes differ, first at %d: %r vs %r" % (what, d.size, d[0], x[d[0]], y[d[0]]))


def _words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        b, k = np.argwhere(got != want)[0]
        raise AssertionError("%s: image %d word %d is %d, expected %d" % (what, b, k, got[b, k], want[b, k]))


@pytest.mark.parametrize("H,W,n", [(1, 1, 3), (37, 53, 3), (64, 64, 3), (375, 1242, 3), (1024, 1920, 1)])
def test_op_flow_score_matches_the_host_entry(hard, H, W, n):
    """Odd H x W: the second plane of every pair and every later image start at an address that is no multiple of 16 bytes (scalar
    loads); 64 x 64 is aligned throughout; one 1024 x 1920 image has more groups than the capped grid has threads (the loop wraps)."""
    fl = F.fields(H, W, n=n)
    flow, gt = fl[0], fl[1]
    for combo in F.combos():
        kw = F.pick(fl, *combo)
        want = ops.flow_score(flow, gt, **kw)
        got = ops.flow_score(flow, gt, model=hard, **kw)
        _words(got, want, "%dx%d valid=%d gt_occ=%d occ_prob=%d" % ((H, W) + combo))
    assert want[:, F.PIXELS:F.PIXELS + 4].sum() > 0 or H * W == 1


def test_device_entry_right_after_compute_flow_device_on_one_stream(soft):
    n, H0, W0 = 2, 130, 200
    V = _clip(3, n + 2, H0, W0, "unit")
    d_ims = [torch.from_numpy(a).cuda() for a in _triplets(V)]
    r = np.random.default_rng(5)
    gt = r.normal(0, 3, (n, 2, H0, W0)).astype(np.float32)
    valid = r.choice(np.array([0, 1, 1, 255], np.uint8), (n, H0, W0))
    occ = r.choice(np.array([0, 1, 1, 2, 3], np.uint8), (n, H0, W0))
    d_gt, d_valid, d_occ = (torch.from_numpy(a).cuda() for a in (gt, valid, occ))
    stream = torch.cuda.Stream()
    for use_valid, use_occ, use_prob in F.combos():
        flow = torch.full((n, 2, H0, W0), 7.0, device="cuda")
        prob = torch.full((n, 2, H0, W0), 7.0, device="cuda")
        scores = torch.full((n, 22), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            soft.computeFlowDevice(*[d.data_ptr() for d in d_ims], n, H0, W0, flow.data_ptr(), d_occ_prob=prob.data_ptr(),
                                   stream=stream.cuda_stream)
            soft.flowScoreDevice(flow.data_ptr(), n, H0, W0, d_gt.data_ptr(), scores.data_ptr(), d_occ_prob=prob.data_ptr() if use_prob else None,
                                 d_valid=d_valid.data_ptr() if use_valid else None, d_gt_occ=d_occ.data_ptr() if use_occ else None,
                                 flow_scale=20.0, stream=stream.cuda_stream)
        stream.synchronize()
        want = ops.flow_score(flow.cpu().numpy(), gt, occ_prob=prob.cpu().numpy() if use_prob else None, valid=valid if use_valid else None,
                              gt_occ=occ if use_occ else None)
        _words(scores.cpu().numpy().view(np.uint64), want, "valid=%d gt_occ=%d occ_prob=%d" % (use_valid, use_occ, use_prob))
    assert want[:, F.PIXELS:F.PIXELS + 4].sum() == n * H0 * W0
    for bad in ("flow", "gt", "scores", "valid"):
        off = lambda name: 4 if name == bad else 0
        with pytest.raises(_lib.B2FError, match="16-byte aligned"):
            soft.flowScoreDevice(flow.data_ptr() + off("flow"), n, H0, W0, d_gt.data_ptr() + off("gt"), scores.data_ptr() + off("scores"),
                                 d_valid=d_valid.data_ptr() + off("valid"))
    with pytest.raises(_lib.B2FError, match="host memory"):
        soft.flowScoreDevice(flow.data_ptr(), n, H0, W0, gt.ctypes.data & ~15, scores.data_ptr())


def _truth(flow, seed, pinned):
    """Ground truth around the estimate, so that the errors fall on both sides of the Fl rule: (gt_flow, valid, gt_occ)"""
    r = np.random.default_rng(seed)
    n, _, H0, W0 = flow.shape
    gt = (flow * np.float32(20.0) + r.normal(0, 2.0, flow.shape) * r.choice([0.1, 1.0, 3.0], (n, 1, H0, W0))).astype(np.float32)
    valid = r.choice(np.array([0, 1, 1, 1, 200], np.uint8), (n, H0, W0))
    gt[:, 0][valid == 0] = 1e9   # Sintel's marker where the mask is off
    occ = r.choice(np.array([0, 1, 1, 1, 2, 3, 255], np.uint8), (n, H0, W0))
    if pinned:
        gt, valid, occ = (torch.from_numpy(a).pin_memory().numpy() for a in (gt, valid, occ))
    return gt, valid, occ


def _buffers(n, H0, W0, pinned):
    def buf(shape, dt):
        t = torch.full(shape, 7, dtype=dt)
        return (t.pin_memory() if pinned else t).numpy()
    return (buf((n, 22), torch.int64).view(np.uint64), buf((n, 2, H0, W0), torch.float32), buf((n, 1, H0, W0), torch.uint8),
            buf((n, 1, H0, W0), torch.uint8))


@pytest.mark.parametrize("which", ["hard", "soft", "trained"])
@pytest.mark.parametrize("H0,W0", [(128, 192), (150, 250)])
@pytest.mark.parametrize("kind", ["u8", "unit"])
def test_compute_flow_score_entries(request, which, H0, W0, kind):
    m = request.getfixturevalue(which)
    T = 7
    n = T - 2
    V = _clip(H0 + len(which), T, H0, W0, kind)
    ims = _triplets(V)
    flow, fo, bo, prob = m.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    gt, valid, occ = _truth(flow, H0 + W0, False)
    want = ops.flow_score(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ)
    s = back2future.score_summary(want)
    print("%s %dx%d %s: epe %.3f px, fl %.3f, oacc %.3f, %d pixels" % (which, H0, W0, kind, s["epe"], s["fl"], s["oacc"], s["pixels"]), flush=True)
    assert 0.0 < s["fl"] < 1.0 and s["pixels"] > 0 and want[:, F.OCC:F.OCC + 9].sum() > 0
    what = "%s %dx%d %s" % (which, H0, W0, kind)
    # one sub-batch
    _words(m.computeFlowSequenceScore(V, gt, valid=valid, gt_occ=occ), want, what + " sequence")
    # fewer planes: the same words as the op gives without them
    _words(m.computeFlowSequenceScore(V, gt), ops.flow_score(flow, gt), what + " sequence, gt_flow alone")
    _words(m.computeFlowBatchScore(*ims, gt, gt_occ=occ), ops.flow_score(flow, gt, occ_prob=prob, gt_occ=occ), what + " batch, no mask")
    _words(m.computeFlowSequenceScore(V, gt, valid=valid, flow_scale=1.0), ops.flow_score(flow, gt, valid=valid, flow_scale=1.0),
           what + " sequence, flow_scale = 1")
    # a 7-frame clip cut into several sub-batches (4 frames = 2 triplets of a sequence, 4 triplets of a batch)
    with m.options(host_subbatch_pixels=4 * H0 * W0):
        _words(m.computeFlowSequenceScore(V, gt, valid=valid, gt_occ=occ), want, what + " sub-batched sequence")
        _words(m.computeFlowBatchScore(*ims, gt, valid=valid, gt_occ=occ), want, what + " the triplets as a batch")
        for pinned in (False, True):
            gt_p, valid_p, occ_p = _truth(flow, H0 + W0, pinned)
            out = _buffers(n, H0, W0, pinned)
            for call in (lambda: m.computeFlowSequenceScore(V, gt_p, valid=valid_p, gt_occ=occ_p, want_flow=True, want_masks=True, out=out),
                         lambda: m.computeFlowBatchScore(*ims, gt_p, valid=valid_p, gt_occ=occ_p, want_flow=True, want_masks=True, out=out)):
                for a in out:
                    a[...] = 7
                res = call()
                assert len(res) == 4 and all(a is b for a, b in zip(res, out))
                _words(res[0], want, "%s pinned=%d all outputs: scores" % (what, pinned))
                for a, b, nm in zip(res[1:], (flow, fo, bo), ("flow", "fwd_occ", "bwd_occ")):
                    _eq(a, b, "%s pinned=%d all outputs: %s" % (what, pinned, nm))
            # scores alone, and scores with the masks alone, into the same kind of memory
            res = m.computeFlowSequenceScore(V, gt_p, valid=valid_p, gt_occ=occ_p, out=out[0])
            assert res is out[0]
            _words(res, want, what + " pinned=%d scores alone" % pinned)
            res = m.computeFlowBatchScore(*ims, gt_p, valid=valid_p, gt_occ=occ_p, want_masks=True, out=(out[0],) + out[2:])
            _words(res[0], want, what + " pinned=%d scores and masks" % pinned)
            for a, b, nm in zip(res[1:], (fo, bo), ("fwd_occ", "bwd_occ")):
                _eq(a, b, "%s pinned=%d scores and masks: %s" % (what, pinned, nm))
    # the f32 entries are what they were
    again = m.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    for a, b in zip(again, (flow, fo, bo, prob)):
        _eq(a, b, "the f32 entry after the score calls")


def test_refusals_with_a_context(hard):
    V = _clip(2, 3, 64, 64, "unit")
    gt = np.zeros((1, 2, 64, 64), np.float32)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            hard.computeFlowSequenceScore(V, gt, flow_scale=scale)
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            ops.flow_score(gt, gt, flow_scale=scale, model=hard)
    d_gt = torch.zeros((1, 2, 64, 64), device="cuda")
    scores = np.zeros((1, 22), np.uint64)
    rc = _lib.lib().b2f_compute_flow_sequence_score(hard._h, 3, back2future.IN_UNIT, V.ctypes.data, 64, 64, 20.0,
                                                     _lib.C.cast(d_gt.data_ptr(), _lib.c_float_p), None, None,
                                                     scores.ctypes.data_as(_lib.C.POINTER(_lib.C.c_ulonglong)), None, None, None)
    assert rc != 0 and "device memory passed to a host-buffer entry point" in _lib.lib().b2f_last_error().decode()
    # a context made with b2f_init_ex options runs the batch entry and refuses the sequence entry, as for f32
    ex = back2future.Model("random:hard", graph="win=5")
    try:
        V4 = _clip(5, 4, 130, 200, "unit")
        ims = _triplets(V4)
        flow = ex.computeFlowBatch(*ims, dtype=np.float32)[0]
        gt4, valid4, _ = _truth(flow, 3, False)
        _words(ex.computeFlowBatchScore(*ims, gt4, valid=valid4), ops.flow_score(flow, gt4, valid=valid4), "a generic-graph context's batch")
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            ex.computeFlowSequenceScore(V4, gt4)
    finally:
        ex.close()


def test_multi_score_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) and a T = 6 sequence on two replicas of one GPU give one context's words."""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    H0, W0 = 100, 150
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        assert mm.n_gpus == 2
        for kind in ("unit", "u8"):
            V = _clip(90, 5, H0, W0, kind)
            ims = _triplets(V)
            flow, fo, bo, prob = ref.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True)
            gt, valid, occ = _truth(flow, 7, False)
            got = mm.computeFlowBatchScore(*ims, gt, valid=valid, gt_occ=occ, want_flow=True, want_masks=True)
            exp = ref.computeFlowBatchScore(*ims, gt, valid=valid, gt_occ=occ, want_flow=True, want_masks=True)
            assert len(got) == len(exp) == 4 and got[0].shape == (3, 22)
            for a, b in zip(got, exp):
                _eq(a, b, "batch " + kind)
            _words(got[0], ops.flow_score(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ), "batch vs the op " + kind)
            for a, b, nm in zip(got[1:], (flow, fo, bo), ("flow", "fwd_occ", "bwd_occ")):
                _eq(a, b, "batch %s: %s" % (kind, nm))
            V6 = _clip(91, 6, H0, W0, kind)
            flow6, _, _, prob6 = ref.computeFlowSequence(V6, dtype=np.float32, occ_prob=True)
            gt6, valid6, occ6 = _truth(flow6, 8, False)
            got6 = mm.computeFlowSequenceScore(V6, gt6, valid=valid6, gt_occ=occ6)
            _words(got6, ref.computeFlowSequenceScore(V6, gt6, valid=valid6, gt_occ=occ6), "sequence " + kind)
            _words(got6, ops.flow_score(flow6, gt6, occ_prob=prob6, valid=valid6, gt_occ=occ6), "sequence vs the op " + kind)
    finally:
        mm.close()
        ref.close()


def test_evaluate_example_prints_the_summary(tmp_path, soft):
    """examples/evaluate.py on four 70 x 130 PNGs with .flo ground truth, masks and occlusion pictures: the summary of
    computeFlowSequenceScore, value for value."""
    from PIL import Image
    r = np.random.default_rng(12)
    src, gtd = tmp_path / "frames", tmp_path / "gt"
    src.mkdir()
    gtd.mkdir()
    for t in range(4):
        Image.fromarray(r.integers(0, 256, (70, 130, 3), dtype=np.uint8)).save(str(src / ("f%02d.png" % t)))
    frames = np.stack([flow_io.load_image(str(src / ("f%02d.png" % t))) for t in range(4)])
    gt = r.normal(0, 4, (2, 2, 70, 130)).astype(np.float32)
    valid = (r.random((2, 70, 130)) < 0.9).astype(np.uint8)
    grey = r.choice(np.array([0, 128, 128, 255, 60], np.uint8), (2, 70, 130))
    occ = np.select([grey == 0, grey == 128, grey == 255], [0, 1, 2], 255).astype(np.uint8)
    script = os.path.join(ROOT, "examples", "evaluate.py")

    def run():
        p = subprocess.run([sys.executable, script, str(src), str(gtd), "random:soft:5:2.0"], check=True, timeout=300, capture_output=True)
        return dict(line.split(" ", 1) for line in p.stdout.decode().splitlines())

    def same(printed, scores):
        want = back2future.score_summary(scores)
        assert set(printed) == set(want)
        for k, v in want.items():
            assert printed[k] == repr(v), (k, printed[k], v)

    for i in range(2):
        flow_io.writeFLO(str(gtd / ("f%02d.flo" % (i + 1))), gt[i])
    same(run(), soft.computeFlowSequenceScore(frames, gt))
    for i in range(2):
        Image.fromarray(valid[i] * 255).save(str(gtd / ("f%02d_valid.png" % (i + 1))))
        Image.fromarray(grey[i]).save(str(gtd / ("f%02d_occ.png" % (i + 1))))
    printed = run()
    same(printed, soft.computeFlowSequenceScore(frames, gt, valid=valid, gt_occ=occ))
    assert int(printed["pixels"]) == int(valid.sum()) and printed["oacc"] != "nan"
