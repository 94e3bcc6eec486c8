"""GPU: motion compensation as an output stage.  b2f_op_flow_warp against the host entry b2f_flow_warp_host (which
tests/test_flow_warp_cpu.py holds against oracle.warping_unit and a numpy restatement): warped bytes / float bits and all 14 words of
every record equal -- the warp is correctly rounded fp32 without contraction and the sums are integers, so no tolerance is involved.
Everything above the kernel is defined from it: b2f_flow_warp_device and the computeFlow*Warp entries give ops.flow_warp of the
float32 flow and occ_prob the existing f32 entries return and of the caller's frames, however the request is cut."""
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops, weights as W
from tests import flow_warp_fields as F
from tests import trained_like as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MEAN = np.array([0.485, 0.456, 0.406] * 3, np.float32).reshape(1, 9, 1, 1)
STD = np.array([0.229, 0.224, 0.225] * 3, np.float32).reshape(1, 9, 1, 1)


def _clip(seed, T, H0, W0, kind):
    """unit: arbitrary floats; u8: bytes; unit255: the floats k / 255, which cross the link as bytes"""
    r = np.random.default_rng(seed)
    if kind == "unit":
        return r.random((T, 3, H0, W0), dtype=np.float32)
    v = r.integers(0, 256, (T, 3, H0, W0), dtype=np.uint8)
    return v if kind == "u8" else v.astype(np.float32) / np.float32(255)


def _triplets(V):
    return [np.ascontiguousarray(a) for a in (V[:-2], V[1:-1], V[2:])]


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def trained():
    """A Soft model with weights like trained ones (tests/trained_like.py), so that the flows span many pixels (x 20: raw units)"""
    r = np.random.default_rng(1)
    V = r.random((3, 3, 128, 192), dtype=np.float32)
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


@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("H,W,n", [(1, 1, 3), (37, 53, 3), (64, 64, 3), (375, 1242, 3), (1024, 1920, 1)])
def test_op_flow_warp_matches_the_host_entry(hard, H, W, n, kind):
    """Odd H x W: rows and planes start at addresses that are no multiple of 16 (or 4) bytes (scalar loads and stores) and rows end in
    a partial group; 64 x 64 is aligned throughout; one 1024 x 1920 image has more groups than the capped grid has threads (the
    loop wraps).  The fields hold whole-pixel and zero flows, targets off every side and exactly on the border, NaN and Inf."""
    flow, ims, prob = F.fields(H, W, n=n, kind=kind)
    what = "%dx%d %s" % (H, W, kind)
    for use_prob in (True, False):
        p = prob if use_prob else None
        w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=p)
        w_got, p_got = ops.flow_warp(flow, *ims, occ_prob=p, model=hard)
        _eq(w_got, w_want, "%s occ_prob=%d: warped" % (what, use_prob))
        _words(p_got, p_want, "%s occ_prob=%d" % (what, use_prob))
        w_only, none_p = ops.flow_warp(flow, *ims, occ_prob=p, want_photo=False, model=hard)
        none_w, p_only = ops.flow_warp(flow, *ims, occ_prob=p, want_warped=False, model=hard)
        assert none_p is None and none_w is None
        _eq(w_only, w_want, "%s occ_prob=%d: warped alone" % (what, use_prob))
        _words(p_only, p_want, "%s occ_prob=%d: photo alone" % (what, use_prob))
    assert p_want[:, F.INSIDE:F.INSIDE + 2].sum() > 0 or H * W == 1


@pytest.mark.parametrize("kind", ["unit", "u8"])
def test_device_entry_right_after_compute_flow_device_on_one_stream(hard, kind):
    n, H0, W0 = 2, 130, 200
    V = _clip(3, n + 2, H0, W0, kind)
    ims = _triplets(V)
    d_ims = [torch.from_numpy(a).cuda() for a in ims]
    stream = torch.cuda.Stream()
    wdt = torch.uint8 if kind == "u8" else torch.float32
    for use_prob, use_warped, use_photo in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
        flow = torch.full((n, 2, H0, W0), 7.0, device="cuda")
        prob = torch.full((n, 2, H0, W0), 7.0, device="cuda")
        warped = torch.full((n, 2, 3, H0, W0), 7, dtype=wdt, device="cuda")
        photo = torch.full((n, 14), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hard.computeFlowDevice(*[d.data_ptr() for d in d_ims], n, H0, W0, flow.data_ptr(), d_occ_prob=prob.data_ptr(),
                                   stream=stream.cuda_stream)
            hard.flowWarpDevice(flow.data_ptr(), n, H0, W0, *[d.data_ptr() for d in d_ims], d_warped=warped.data_ptr() if use_warped else None,
                                d_photo=photo.data_ptr() if use_photo else None, d_occ_prob=prob.data_ptr() if use_prob else None,
                                as_bytes=kind == "u8", stream=stream.cuda_stream)
        stream.synchronize()
        w_want, p_want = ops.flow_warp(flow.cpu().numpy(), *ims, occ_prob=prob.cpu().numpy() if use_prob else None)
        what = "%s occ_prob=%d warped=%d photo=%d" % (kind, use_prob, use_warped, use_photo)
        if use_warped:
            _eq(warped.cpu().numpy(), w_want, what)
        if use_photo:
            _words(photo.cpu().numpy().view(np.uint64), p_want, what)
    for bad in ("flow", "im2", "warped", "photo"):
        off = lambda name: 4 if name == bad else 0
        with pytest.raises(_lib.B2FError, match="16-byte aligned"):
            hard.flowWarpDevice(flow.data_ptr() + off("flow"), n, H0, W0, d_ims[0].data_ptr(), d_ims[1].data_ptr() + off("im2"), d_ims[2].data_ptr(),
                                d_warped=warped.data_ptr() + off("warped"), d_photo=photo.data_ptr() + off("photo"), as_bytes=kind == "u8")
    with pytest.raises(_lib.B2FError, match="host memory"):
        hard.flowWarpDevice(flow.data_ptr(), n, H0, W0, d_ims[0].data_ptr(), ims[1].ctypes.data & ~15, d_ims[2].data_ptr(), d_photo=photo.data_ptr(),
                            as_bytes=kind == "u8")
    with pytest.raises(_lib.B2FError, match="at least one of warped and photo"):
        hard.flowWarpDevice(flow.data_ptr(), n, H0, W0, *[d.data_ptr() for d in d_ims], as_bytes=kind == "u8")


def _buffers(n, H0, W0, as_bytes, pinned):
    """(warped, photo, flow, fwd_occ, bwd_occ, occ_prob) filled with sevens"""
    def buf(shape, dt):
        t = torch.full(shape, 7, dtype=dt)
        return (t.pin_memory() if pinned else t).numpy()
    return (buf((n, 2, 3, H0, W0), torch.uint8 if as_bytes else torch.float32), buf((n, 14), torch.int64).view(np.uint64),
            buf((n, 2, H0, W0), torch.float32), buf((n, 1, H0, W0), torch.uint8), buf((n, 1, H0, W0), torch.uint8),
            buf((n, 2, H0, W0), torch.float32))


@pytest.mark.parametrize("which", ["hard", "trained"])
@pytest.mark.parametrize("H0,W0", [(128, 192), (150, 250)])
@pytest.mark.parametrize("kind", ["u8", "unit", "unit255"])
def test_compute_flow_warp_entries(request, which, H0, W0, kind):
    """u8 frames are sampled as floats after the upload (batches, rescaled sizes) or as the bytes themselves (a /64 sequence);
    unit255 frames cross the link as bytes and come back as floats: all four (byte | float in) x (byte | float out) kernels run."""
    m = request.getfixturevalue(which)
    T = 7
    n = T - 2
    V = _clip(H0 + len(which), T, H0, W0, kind)
    ims = _triplets(V)
    flow, fo, bo, prob = m.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=prob)
    s = back2future.photo_summary(p_want)
    displaced = float((np.hypot(flow[:, 0].astype(np.float64), flow[:, 1].astype(np.float64)) * 20.0 >= 1.0).mean())
    outside = p_want[:, F.OUTSIDE:F.OUTSIDE + 2].sum(axis=0)
    print("%s %dx%d %s: pme %.4f, bc %.4f, psnr %.2f / %.2f dB, inside %.3f / %.3f, displaced >= 1 px %.3f, outside %d / %d" %
          (which, H0, W0, kind, s["pme"], s["bc"], s["psnr_past"], s["psnr_future"], s["inside_past"], s["inside_future"], displaced,
           outside[0], outside[1]), flush=True)
    if which == "trained":   # the stage must not be tested on flows that move nothing
        assert displaced >= 0.5 and outside[0] > 0 and outside[1] > 0
    what = "%s %dx%d %s" % (which, H0, W0, kind)
    # one sub-batch
    w, p = m.computeFlowSequenceWarp(V)
    _eq(w, w_want, what + " sequence: warped")
    _words(p, p_want, what + " sequence")
    w, p = m.computeFlowBatchWarp(*ims)
    _eq(w, w_want, what + " batch: warped")
    _words(p, p_want, what + " batch")
    _words(m.computeFlowSequenceWarp(V, want_warped=False), p_want, what + " sequence, photo alone")
    _eq(m.computeFlowBatchWarp(*ims, want_photo=False), w_want, what + " batch, warped alone")
    _words(m.computeFlowSequenceWarp(V, flow_scale=1.0, want_warped=False), ops.flow_warp(flow, *ims, occ_prob=prob, flow_scale=1.0, want_warped=False)[1],
           what + " sequence, flow_scale = 1")
    # a 7-frame clip cut into several sub-batches (4 frames = 2 triplets of a sequence, 4 triplets of a batch)
    with m.options(host_subbatch_pixels=4 * H0 * W0):
        w, p = m.computeFlowSequenceWarp(V)
        _eq(w, w_want, what + " sub-batched sequence: warped")
        _words(p, p_want, what + " sub-batched sequence")
        w, p = m.computeFlowBatchWarp(*ims)
        _eq(w, w_want, what + " the triplets as a batch: warped")
        _words(p, p_want, what + " the triplets as a batch")
        for pinned in (False, True):
            out = _buffers(n, H0, W0, kind == "u8", pinned)
            for call in (lambda: m.computeFlowSequenceWarp(V, want_flow=True, want_masks=True, want_prob=True, out=out),
                         lambda: m.computeFlowBatchWarp(*ims, want_flow=True, want_masks=True, want_prob=True, out=out)):
                for a in out:
                    a[...] = 7
                res = call()
                assert len(res) == 6 and all(a is b for a, b in zip(res, out))
                _words(res[1], p_want, "%s pinned=%d all outputs: photo" % (what, pinned))
                for a, b, nm in zip((res[0],) + res[2:], (w_want, flow, fo, bo, prob), ("warped", "flow", "fwd_occ", "bwd_occ", "occ_prob")):
                    _eq(a, b, "%s pinned=%d all outputs: %s" % (what, pinned, nm))
            # the photo alone, and warped frames with the masks alone, into the same kind of memory
            out[1][...] = 7
            res = m.computeFlowSequenceWarp(V, want_warped=False, out=out[1])
            assert res is out[1]
            _words(res, p_want, what + " pinned=%d photo alone" % pinned)
            out[0][...] = 7
            res = m.computeFlowBatchWarp(*ims, want_photo=False, want_masks=True, out=(out[0], out[3], out[4]))
            for a, b, nm in zip(res, (w_want, fo, bo), ("warped", "fwd_occ", "bwd_occ")):
                _eq(a, b, "%s pinned=%d warped and masks: %s" % (what, pinned, nm))
    # the f32 entries are what they were
    again = m.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    for a, b in zip(again, (flow, fo, bo, prob)):
        _eq(a, b, "the f32 entry after the warp calls")


def test_refusals_with_a_context(hard):
    V = _clip(2, 3, 64, 64, "unit")
    flow = np.zeros((1, 2, 64, 64), np.float32)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            hard.computeFlowSequenceWarp(V, flow_scale=scale)
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            hard.computeFlowBatchWarp(*_triplets(V), flow_scale=scale)
        with pytest.raises(_lib.B2FError, match="flow_scale"):
            ops.flow_warp(flow, V[:1], V[1:2], V[2:], flow_scale=scale, model=hard)
    L = _lib.lib()
    photo = np.zeros((1, 14), np.uint64)
    pp = photo.ctypes.data_as(_lib.C.POINTER(_lib.C.c_ulonglong))
    # neither output
    rc = L.b2f_compute_flow_sequence_warp(hard._h, 3, back2future.IN_UNIT, V.ctypes.data, 64, 64, 20.0, None, None, None, None, None, None)
    assert rc != 0 and "at least one of warped and photo" in L.b2f_last_error().decode()
    # device memory where host buffers belong
    d_w = torch.zeros((1, 2, 3, 64, 64), device="cuda")
    rc = L.b2f_compute_flow_sequence_warp(hard._h, 3, back2future.IN_UNIT, V.ctypes.data, 64, 64, 20.0, d_w.data_ptr(), pp, None, None, None, None)
    assert rc != 0 and "device memory passed to a host-buffer entry point" in L.b2f_last_error().decode()
    # a stream has no warp entry: its pushes take the f32 and rgb outputs alone
    assert not any("warp" in name.lower() for name in dir(back2future.FlowStream))
    # a context made with b2f_init_ex options runs the batch entry and refuses the sequence entry, as for f32
    ex = back2future.Model("random:hard", graph="win=5")
    try:
        V4 = _clip(5, 4, 130, 200, "u8")
        ims = _triplets(V4)
        flow4, _, _, prob4 = ex.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True)
        w_want, p_want = ops.flow_warp(flow4, *ims, occ_prob=prob4)
        w, p = ex.computeFlowBatchWarp(*ims)
        _eq(w, w_want, "a generic-graph context's batch: warped")
        _words(p, p_want, "a generic-graph context's batch")
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            ex.computeFlowSequenceWarp(V4)
    finally:
        ex.close()


def test_multi_warp_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) and a T = 6 sequence on two replicas of one GPU give one context's bytes and words."""
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
            got = mm.computeFlowBatchWarp(*ims, want_flow=True, want_masks=True, want_prob=True)
            exp = ref.computeFlowBatchWarp(*ims, want_flow=True, want_masks=True, want_prob=True)
            assert len(got) == len(exp) == 6 and got[1].shape == (3, 14)
            for a, b in zip(got, exp):
                _eq(a, b, "batch " + kind)
            w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=prob)
            _words(got[1], p_want, "batch vs the op " + kind)
            for a, b, nm in zip((got[0],) + got[2:], (w_want, flow, fo, bo, prob), ("warped", "flow", "fwd_occ", "bwd_occ", "occ_prob")):
                _eq(a, b, "batch %s: %s" % (kind, nm))
            V6 = _clip(91, 6, H0, W0, kind)
            flow6, _, _, prob6 = ref.computeFlowSequence(V6, dtype=np.float32, occ_prob=True)
            w6, p6 = mm.computeFlowSequenceWarp(V6)
            r6 = ref.computeFlowSequenceWarp(V6)
            _eq(w6, r6[0], "sequence %s: warped" % kind)
            _words(p6, r6[1], "sequence " + kind)
            w_want6, p_want6 = ops.flow_warp(flow6, *_triplets(V6), occ_prob=prob6)
            _eq(w6, w_want6, "sequence vs the op %s: warped" % kind)
            _words(p6, p_want6, "sequence vs the op " + kind)
    finally:
        mm.close()
        ref.close()


def test_compensate_example_writes_the_warped_frames(tmp_path):
    """examples/compensate.py on five 128 x 192 PNGs: its pictures are computeFlowSequenceWarp's bytes and its printed summary is
    photo_summary of that call's records, value for value; --no-images prints the same summary and writes nothing."""
    from PIL import Image
    r = np.random.default_rng(12)
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    names = ["f%02d" % t for t in range(5)]
    frames = r.integers(0, 256, (5, 128, 192, 3), dtype=np.uint8)
    for nm, f in zip(names, frames):
        Image.fromarray(f).save(str(src / (nm + ".png")))
    script = os.path.join(ROOT, "examples", "compensate.py")

    def run(*extra):
        p = subprocess.run([sys.executable, script, str(src), str(dst), "random:soft:5:2.0"] + list(extra), check=True, timeout=300,
                           capture_output=True)
        return dict(line.split(" ", 1) for line in p.stdout.decode().splitlines())

    m = back2future.Model("random:soft:5:2.0")
    try:
        warped, photo = m.computeFlowSequenceWarp(np.ascontiguousarray(frames.transpose(0, 3, 1, 2)))
    finally:
        m.close()
    want = back2future.photo_summary(photo)
    printed = run("--no-images")
    assert not dst.exists()
    assert set(printed) == set(want)
    for k, v in want.items():
        assert printed[k] == repr(v), (k, printed[k], v)
    assert run() == printed
    assert sorted(os.listdir(str(dst))) == sorted(nm + tail for nm in names[1:-1] for tail in ("_past.png", "_future.png"))
    for i, nm in enumerate(names[1:-1]):
        for d, tail in enumerate(("_past.png", "_future.png")):
            pic = np.asarray(Image.open(str(dst / (nm + tail))), np.uint8).transpose(2, 0, 1)
            _eq(pic, warped[i, d], nm + tail)
