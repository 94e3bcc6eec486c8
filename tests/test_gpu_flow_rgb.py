"""GPU: flow pictures (xy2rgb as an output stage).  b2f_op_flow_rgb against the host entry b2f_flow_rgb_host (which
tests/test_flow_rgb_cpu.py holds against flow_io.xy2rgb): no byte more than 1 level away, at most 1e-6 of the bytes different, the
maxima bit-equal.  Everything above the kernel is defined from it bit for bit: b2f_flow_rgb_device and the computeFlow*RGB entries
give b2f_op_flow_rgb of the float32 flow the existing f32 entries return."""
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, flow_io, ops, weights as W
from tests import trained_like as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_LEVELS = 1
MAX_SHARE = 1e-6
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


def _close(got, want, what):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    levels, differing = int(d.max()), int((d > 0).sum())
    print("%s: largest byte difference %d, %d of %d bytes differ (%.2e)" % (what, levels, differing, d.size, differing / d.size), flush=True)
    assert levels <= MAX_LEVELS, what
    assert differing <= MAX_SHARE * d.size, what


def field_a(H=1024, W=1920, seed=0):
    """The field of tests/test_flow_rgb_cpu.py: sines up to 30 px plus noise, rows of exact x == 0, y == 0 and zero flow."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    x = (30 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + rng.normal(0, 2, (H, W))).astype(np.float32)
    y = (12 * np.cos(xx / 45.0) + rng.normal(0, 2, (H, W))).astype(np.float32)
    x[:8] = 0
    y[8:16] = 0
    x[16:20] = 0
    y[16:20] = 0
    return np.stack([x, y])[None]


def _small_field(H, W):
    """n = 3 images of very different magnitudes, with exact zeros on the axes"""
    r = np.random.default_rng(H * 1000 + W)
    f = r.normal(0, 1, (3, 2, H, W)).astype(np.float32) * np.array([1e-3, 3.0, 50.0], np.float32)[:, None, None, None]
    f[:, 0, ::3, ::5] = 0
    f[:, 1, ::4, ::5] = 0
    return f


@pytest.mark.parametrize("H,W", [(1024, 1920), (1, 1), (37, 53), (375, 1242)])
def test_op_flow_rgb_matches_the_host_entry(hard, H, W):
    flow = field_a() if (H, W) == (1024, 1920) else _small_field(H, W)
    for mx in (None, 20.0):
        for packed in (False, True):
            want, want_max = ops.flow_rgb(flow, max=mx, packed=packed)
            got, got_max = ops.flow_rgb(flow, max=mx, packed=packed, model=hard)
            assert got.shape == want.shape and got.dtype == np.uint8
            _close(got, want, "%dx%d max=%r packed=%r" % (H, W, mx, packed))
            _eq(got_max, want_max, "%dx%d max=%r max_used" % (H, W, mx))


def test_device_entry_right_after_compute_flow_device_on_one_stream(hard):
    n, H0, W0 = 2, 130, 200
    V = _clip(3, n + 2, H0, W0, "unit")
    d_ims = [torch.from_numpy(a).cuda() for a in _triplets(V)]
    stream = torch.cuda.Stream()
    for mx in (None, 0.05):
        for packed in (False, True):
            for own_max in (True, False):
                flow = torch.full((n, 2, H0, W0), 7.0, device="cuda")
                rgb = torch.full((n, H0, W0, 3) if packed else (n, 3, H0, W0), 7, dtype=torch.uint8, device="cuda")
                used = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if own_max else None
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    hard.computeFlowDevice(*[d.data_ptr() for d in d_ims], n, H0, W0, flow.data_ptr(), stream=stream.cuda_stream)
                    hard.flowRGBDevice(flow.data_ptr(), n, H0, W0, rgb.data_ptr(), max=mx, packed=packed,
                                       d_max_used=used.data_ptr() if own_max else None, stream=stream.cuda_stream)
                stream.synchronize()
                want, want_max = ops.flow_rgb(flow.cpu().numpy(), max=mx, packed=packed, model=hard)
                what = "max=%r packed=%r own_max=%r" % (mx, packed, own_max)
                _eq(rgb.cpu().numpy(), want, what)
                if own_max:
                    _eq(used.cpu().numpy(), want_max, what + " max_used")
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        hard.flowRGBDevice(flow.data_ptr() + 4, n, H0, W0, rgb.data_ptr())
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        hard.flowRGBDevice(flow.data_ptr(), n, H0, W0, rgb.data_ptr() + 4)


def _buffers(n, H0, W0, packed, pinned):
    def buf(shape, dt):
        t = torch.full(shape, 7, dtype=dt)
        return (t.pin_memory() if pinned else t).numpy()
    return (buf((n, H0, W0, 3) if packed else (n, 3, H0, W0), torch.uint8), buf((n,), torch.float64), buf((n, 2, H0, W0), torch.float32),
            buf((n, 1, H0, W0), torch.uint8), buf((n, 1, H0, W0), torch.uint8))


@pytest.mark.parametrize("which", ["hard", "soft", "trained"])
@pytest.mark.parametrize("H0,W0", [(128, 192), (150, 250)])
@pytest.mark.parametrize("kind", ["u8", "unit"])
def test_compute_flow_rgb_entries(request, which, H0, W0, kind):
    m = request.getfixturevalue(which)
    T = 7
    n = T - 2
    V = _clip(H0 + len(which), T, H0, W0, kind)
    ims = _triplets(V)
    flow, fo, bo = m.computeFlowSequence(V, dtype=np.float32)
    flow_b, fo_b, bo_b = m.computeFlowBatch(*ims, dtype=np.float32)
    _eq(flow_b, flow, "the f32 entries agree")
    span = float(np.sqrt((flow.astype(np.float64) ** 2).sum(1)).max())
    print("%s %dx%d %s: largest raw flow %.3f (x 20 = %.1f px)" % (which, H0, W0, kind, span, 20 * span), flush=True)
    if which == "trained":
        # computeFlow returns the raw network flow, pixels / 20 (back2future.lua:77-84); calibrate() gives the flow heads a
        # deviation of 0.25, i.e. 5 px, so the largest vector of a clip is well beyond that
        assert 20 * span > 5.0, "the trained-like weights should give flows of several pixels"
    for mx, packed in ((None, False), (None, True), (0.5 * span, True), (0.5 * span, False)):
        what = "%s %dx%d %s max=%r packed=%r" % (which, H0, W0, kind, mx, packed)
        want, want_max = ops.flow_rgb(flow, max=mx, packed=packed, model=m)
        # one sub-batch
        rgb, used = m.computeFlowSequenceRGB(V, max=mx, packed=packed)
        _eq(rgb, want, what + " sequence")
        _eq(used, want_max, what + " sequence max_used")
        # a 7-frame clip cut into several sub-batches (4 frames = 2 triplets of a sequence, 4 triplets of a batch)
        with m.options(host_subbatch_pixels=4 * H0 * W0):
            rgb, used = m.computeFlowSequenceRGB(V, max=mx, packed=packed)
            _eq(rgb, want, what + " sub-batched sequence")
            _eq(used, want_max, what + " sub-batched sequence max_used")
            rgb_b, used_b = m.computeFlowBatchRGB(*ims, max=mx, packed=packed)
            _eq(rgb_b, rgb, what + " the triplets as a batch")
            _eq(used_b, used, what + " the triplets as a batch, max_used")
            for pinned in (False, True):
                out = _buffers(n, H0, W0, packed, pinned)
                for call in (lambda: m.computeFlowSequenceRGB(V, max=mx, packed=packed, want_flow=True, want_masks=True, out=out),
                             lambda: m.computeFlowBatchRGB(*ims, max=mx, packed=packed, want_flow=True, want_masks=True, out=out)):
                    for a in out:
                        a[...] = 7
                    res = call()
                    assert len(res) == 5 and all(a is b for a, b in zip(res, out))
                    for a, b, nm in zip(res, (want, want_max, flow, fo, bo), ("rgb", "max_used", "flow", "fwd_occ", "bwd_occ")):
                        _eq(a, b, "%s pinned=%d all outputs: %s" % (what, pinned, nm))
                # pictures alone, and pictures with the masks alone, into the same kind of memory
                res = m.computeFlowSequenceRGB(V, max=mx, packed=packed, out=out[:2])
                _eq(res[0], want, what + " pinned=%d pictures alone" % pinned)
                _eq(res[1], want_max, what + " pinned=%d pictures alone, max_used" % pinned)
                res = m.computeFlowBatchRGB(*ims, max=mx, packed=packed, want_masks=True, out=out[:2] + out[3:])
                for a, b, nm in zip(res, (want, want_max, fo, bo), ("rgb", "max_used", "fwd_occ", "bwd_occ")):
                    _eq(a, b, "%s pinned=%d pictures and masks: %s" % (what, pinned, nm))
    # the f32 entries are what they were
    again = m.computeFlowSequence(V, dtype=np.float32)
    for a, b in zip(again, (flow, fo, bo)):
        _eq(a, b, "the f32 entry after the rgb calls")


def test_multi_rgb_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) and a T = 6 sequence on two replicas of one GPU give one context's bytes."""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    H0, W0 = 100, 150
    mm = back2future.MultiModel("random:hard:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:hard:5:2.0")
    try:
        assert mm.n_gpus == 2
        for kind in ("unit", "u8"):
            V = _clip(90, 5, H0, W0, kind)
            ims = _triplets(V)
            V6 = _clip(91, 6, H0, W0, kind)
            for mx, packed in ((None, False), (0.05, True)):
                what = "%s max=%r packed=%r" % (kind, mx, packed)
                got = mm.computeFlowBatchRGB(*ims, max=mx, packed=packed, want_flow=True, want_masks=True)
                exp = ref.computeFlowBatchRGB(*ims, max=mx, packed=packed, want_flow=True, want_masks=True)
                assert len(got) == len(exp) == 5 and got[0].shape[0] == 3
                for a, b in zip(got, exp):
                    _eq(a, b, "batch " + what)
                flow = ref.computeFlowBatch(*ims, dtype=np.float32)[0]
                _eq(got[0], ops.flow_rgb(flow, max=mx, packed=packed, model=ref)[0], "batch vs the op " + what)
                for a, b in zip(mm.computeFlowSequenceRGB(V6, max=mx, packed=packed), ref.computeFlowSequenceRGB(V6, max=mx, packed=packed)):
                    _eq(a, b, "sequence " + what)
    finally:
        mm.close()
        ref.close()


def test_run_sequence_example_writes_the_pictures(tmp_path, soft):
    """examples/run_sequence.py --rgb [MAX]: one PNG per centre frame, the packed picture of computeFlowSequenceRGB; .flo files and
    masks only with --flo, and then the bytes the example writes without --rgb."""
    from PIL import Image
    r = np.random.default_rng(12)
    src = tmp_path / "frames"
    src.mkdir()
    for t in range(4):
        Image.fromarray(r.integers(0, 256, (70, 130, 3), dtype=np.uint8)).save(str(src / ("f%02d.png" % t)))
    frames = np.stack([flow_io.load_image(str(src / ("f%02d.png" % t))) for t in range(4)])
    script = os.path.join(ROOT, "examples", "run_sequence.py")
    for extra, mx, flo in ((["--rgb"], None, False), (["--rgb", "0.3", "--flo"], 0.3, True)):
        out = tmp_path / ("out%d" % flo)
        subprocess.run([sys.executable, script, str(src), str(out), "random:soft:5:2.0"] + extra, check=True, timeout=300, capture_output=True)
        rgb, _, flow, fo, bo = soft.computeFlowSequenceRGB(frames, max=mx, packed=True, want_flow=True, want_masks=True)
        for i in range(2):
            stem = "f%02d" % (i + 1)
            _eq(np.asarray(Image.open(str(out / (stem + "_flow.png")))), rgb[i], stem + " picture")
            assert (out / (stem + ".flo")).exists() == flo and (out / (stem + "_fwd_occ.png")).exists() == flo
            if flo:
                flow_io.writeFLO(str(tmp_path / "ref.flo"), flow[i])
                assert (out / (stem + ".flo")).read_bytes() == (tmp_path / "ref.flo").read_bytes(), stem
