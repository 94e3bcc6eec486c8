"""GPU: flow over a video with one feature pyramid per frame (b2f_forward_sequence_device, b2f_compute_flow_sequence[_u8],
b2f_multi_compute_flow_sequence[_u8]).  Output i of a sequence must be what the triplet entry points return for frames
(i, i+1, i+2) -- bit for bit: the sequence mode only changes where the pyramid's images live, not a single operation."""
import ctypes as C

import numpy as np
import pytest

from back2future_amd import _lib, back2future, weights as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def _frames(seed, T, H, W, kind):
    """(T x 3 x H x W device frames as the sequence entry reads them, the same frames as fp32 for the triplet entry, in_kind)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "u8":
        b = torch.randint(0, 256, (T, 3, H, W), dtype=torch.uint8, generator=g)
        f = torch.from_numpy(b.numpy().astype(np.float32) / np.float32(255))   # correctly rounded k / 255, as image.load
        return b.cuda(), f.cuda(), back2future.IN_U8
    if kind == "unit":
        f = torch.rand((T, 3, H, W), generator=g)
        return f.cuda(), f.cuda(), back2future.IN_UNIT
    f = torch.randn((T, 3, H, W), generator=g)
    return f.cuda(), f.cuda(), back2future.IN_NORMALIZED


def _triplets(f):
    return torch.cat([f[:-2], f[1:-1], f[2:]], dim=1).contiguous()   # (T-2) x 9 x H x W: triplet b = frames b, b+1, b+2


def _outs(m, B, H, W):
    c3 = 2 if m.past_flow else 3
    return [torch.empty((B, c, H, W), device="cuda") for c in (2, 2, c3)]


def _run_triplets(m, x, H, W, unit, outs):
    m.forward_device(x.data_ptr(), x.shape[0], H, W, *[o.data_ptr() for o in outs], unit_input=unit)
    m.synchronize()


def _run_sequence(m, frames, T, H, W, in_kind, outs):
    m.forward_sequence_device(frames.data_ptr(), T, H, W, *[o.data_ptr() for o in outs], in_kind=in_kind)
    m.synchronize()


def _assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: output %d differs (max |d| = %g)" % (what, i, float((x - y).abs().max()))


@pytest.mark.parametrize("which", ["hard", "soft"])
@pytest.mark.parametrize("T,H,W", [(3, 128, 192), (4, 128, 192), (7, 128, 192), (18, 1024, 1920)])
def test_device_sequence_equals_overlapping_triplets(request, which, T, H, W):
    m = request.getfixturevalue(which)
    for seed, kind in enumerate(["unit", "normalized", "u8"]):
        seq_in, f32, in_kind = _frames(100 + seed, T, H, W, kind)
        exp = _outs(m, T - 2, H, W)
        _run_triplets(m, _triplets(f32), H, W, in_kind != back2future.IN_NORMALIZED, exp)
        got = _outs(m, T - 2, H, W)
        _run_sequence(m, seq_in, T, H, W, in_kind, got)
        _assert_same(got, exp, "%s T=%d %dx%d %s" % (which, T, H, W, kind))
        del seq_in, f32, exp, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_graph_cache_keeps_sequence_and_triplet_calls_apart(request, which):
    """use_graph = 1: a sequence call and a triplet call on the same dev_in, B, H and W must each replay their own graph.
    Three rounds (eager, capture, replay), each result equal to its eager counterpart."""
    m = request.getfixturevalue(which)
    T, H, W = 5, 128, 192
    B = T - 2
    _, f, _ = _frames(7, T, H, W, "unit")
    x = _triplets(f)
    exp_t, exp_s = _outs(m, B, H, W), _outs(m, B, H, W)
    _run_triplets(m, x, H, W, True, exp_t)
    _run_sequence(m, f, T, H, W, back2future.IN_UNIT, exp_s)
    buf = torch.empty_like(x)          # B x 9 x H x W: the sequence reads its first T x 3 planes
    outs = _outs(m, B, H, W)
    with m.options(use_graph=1):
        for rnd in range(3):
            for mode in ("seq", "tri"):
                torch.cuda.synchronize()
                if mode == "seq":
                    buf.view(-1)[:f.numel()].copy_(f.reshape(-1))
                else:
                    buf.copy_(x)
                torch.cuda.synchronize()
                if mode == "seq":
                    _run_sequence(m, buf, T, H, W, back2future.IN_UNIT, outs)
                else:
                    _run_triplets(m, buf, H, W, True, outs)
                _assert_same(outs, exp_s if mode == "seq" else exp_t, "round %d, %s call" % (rnd, mode))


def _host_frames(seed, T, H0, W0, kind):
    r = np.random.default_rng(seed)
    if kind == "float32":
        return r.random((T, 3, H0, W0), dtype=np.float32)
    b = r.integers(0, 256, (T, 3, H0, W0), dtype=np.uint8)
    return b if kind == "uint8" else b.astype(np.float32) / np.float32(255)   # exactly k / 255: crosses as bytes


def _batch_of(m, V):
    return m.computeFlowBatch(V[:-2], V[1:-1], V[2:])


@pytest.mark.parametrize("which", ["hard", "soft"])
@pytest.mark.parametrize("H0,W0", [(100, 150), (375, 1242)])
def test_host_sequence_equals_batch_of_triplets(request, which, H0, W0):
    m = request.getfixturevalue(which)
    T = 6
    for seed, kind in enumerate(["float32", "uint8", "k255"]):
        V = _host_frames(10 + seed, T, H0, W0, kind)
        exp = _batch_of(m, V)
        got = m.computeFlowSequence(V)
        for a, b in zip(got, exp):
            assert a.shape == b.shape and a.dtype == b.dtype
            np.testing.assert_array_equal(a, b, err_msg="%s %dx%d %s" % (which, H0, W0, kind))
    # a list of frames is the same call
    V = _host_frames(20, 4, H0, W0, "float32")
    for a, b in zip(m.computeFlowSequence(list(V)), _batch_of(m, V)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ramp", [0, 1])
def test_host_sequence_overlapping_subbatches_and_pinned_buffers(hard, ramp):
    """Several sub-batches (each uploads its frames, the two shared with the next one again), page-locked caller buffers."""
    T, H0, W0 = 11, 100, 150
    for kind in ("float32", "uint8", "k255"):
        V = _host_frames(30, T, H0, W0, kind)
        exp = _batch_of(hard, V)
        with hard.options(host_subbatch_pixels=4 * H0 * W0, host_ramp=ramp):
            got = hard.computeFlowSequence(V)
            pin_in = torch.from_numpy(V).pin_memory()
            pin_out = (torch.empty((T - 2, 2, H0, W0), dtype=torch.float64).pin_memory(),
                       torch.empty((T - 2, 1, H0, W0), dtype=torch.uint8).pin_memory(),
                       torch.empty((T - 2, 1, H0, W0), dtype=torch.uint8).pin_memory())
            got_pin = hard.computeFlowSequence(pin_in.numpy(), out=tuple(t.numpy() for t in pin_out))
        for a, b, c in zip(got, got_pin, exp):
            np.testing.assert_array_equal(a, c, err_msg="ramp %d %s" % (ramp, kind))
            np.testing.assert_array_equal(b, c, err_msg="ramp %d %s pinned" % (ramp, kind))


def test_sequence_vs_oracle(soft):
    T, H, Wd = 5, 64, 128
    r = np.random.default_rng(0)
    V = r.random((T, 3, H, Wd), dtype=np.float32)
    flow, fo, bo = soft.computeFlowSequence(V)
    w = W.random_init(5, True, 2.0)
    for i in range(T - 2):
        eflow, efo, ebo = O.compute_flow(V[i], V[i + 1], V[i + 2], w, True)
        err = float(np.abs(flow[i] - eflow).max())
        assert err <= 1e-3, (i, err)


def test_multi_sequence_two_replicas_on_one_gpu(monkeypatch):
    """The N > 1 path on one GPU (the switches of test_gpu_parity.py::test_multi_gpu_two_replicas_on_one_gpu): the triplets
    are sharded, replica i reads frames [lo, hi + 2); results equal one context's, a replica's failure names its GPU."""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    H0, W0 = 100, 150
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        assert mm.n_gpus == 2
        for T in (5, 12):
            V = _host_frames(40 + T, T, H0, W0, "float32")
            exp = ref.computeFlowSequence(V)
            for a, b in zip(mm.computeFlowSequence(V), exp):
                np.testing.assert_array_equal(a, b, err_msg="T=%d" % T)
            by = _host_frames(50 + T, T, H0, W0, "uint8")
            for a, b in zip(mm.computeFlowSequence(by), ref.computeFlowSequence(by)):
                np.testing.assert_array_equal(a, b, err_msg="T=%d u8" % T)
        L = _lib.lib()
        _lib.check(L.b2f_set_option(C.c_void_p(L.b2f_multi_context(mm._h, 1)), b"debug_fail_next", 1))
        V = _host_frames(60, 5, H0, W0, "float32")
        with pytest.raises(_lib.B2FError, match="GPU 0: .*forced failure"):
            mm.computeFlowSequence(V)
        for a, b in zip(mm.computeFlowSequence(V), ref.computeFlowSequence(V)):
            np.testing.assert_array_equal(a, b)
    finally:
        mm.close()
        ref.close()


def test_sequence_errors(hard):
    L = _lib.lib()
    V = np.zeros((3, 3, 64, 64), np.float32)
    flow = np.zeros((1, 2, 64, 64), np.float64)
    m1, m2 = np.zeros((1, 1, 64, 64), np.uint8), np.zeros((1, 1, 64, 64), np.uint8)
    outp = (flow.ctypes.data_as(C.POINTER(C.c_double)), m1.ctypes.data_as(C.POINTER(C.c_ubyte)),
            m2.ctypes.data_as(C.POINTER(C.c_ubyte)))
    with pytest.raises(_lib.B2FError, match="T >= 3"):
        _lib.check(L.b2f_compute_flow_sequence(hard._h, 2, _lib.fptr(V), 64, 64, *outp))
    d = torch.zeros((3, 3, 64, 64), device="cuda")
    with pytest.raises(_lib.B2FError, match="T >= 3"):
        _lib.check(L.b2f_forward_sequence_device(hard._h, C.c_void_p(d.data_ptr()), 1, 2, 64, 64, None, None, None, None))
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        hard.forward_sequence_device(d.data_ptr() + 4, 3, 64, 64, in_kind=back2future.IN_UNIT)
    out = torch.zeros((1, 2, 64, 64), device="cuda")
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        hard.forward_sequence_device(d.data_ptr(), 3, 64, 64, d_flow=out.data_ptr() + 8, in_kind=back2future.IN_UNIT)
    with pytest.raises(_lib.B2FError, match="in_kind"):
        hard.forward_sequence_device(d.data_ptr(), 3, 64, 64, in_kind=3)
    g = back2future.Model("random:hard", graph="win=5")
    try:
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            g.computeFlowSequence(V)
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            g.forward_sequence_device(d.data_ptr(), 3, 64, 64, in_kind=back2future.IN_UNIT)
    finally:
        g.close()


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_profile_names_the_sequence_kernels(request, which):
    m = request.getfixturevalue(which)
    T, H, W = 4, 128, 192
    seq_in, _, in_kind = _frames(3, T, H, W, "u8")
    outs = _outs(m, T - 2, H, W)
    m.synchronize()
    with m.options(profile=1):
        m.profile_reset()
        _run_sequence(m, seq_in, T, H, W, in_kind, outs)
        rows = m.profile_read()
        m.profile_reset()
    assert "conv_first_seq" in rows and "conv_first" not in rows, sorted(rows)
    if not m.past_flow:
        assert "warp_image_seq" in rows and "warp_image" not in rows, sorted(rows)
