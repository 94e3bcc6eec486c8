"""GPU: FlowStream (b2f_stream_*), frames pushed one at a time with the pyramid features kept on the GPU.  On the default options
push k >= 3 must be output k - 3 of computeFlowSequence(dtype=np.float32, occ_prob=True) on the same frames -- bit for bit: a stream
only changes where the pyramid's images live and how many of them a pyramid launch holds, not a single operation."""
import ctypes as C

import numpy as np
import pytest

from back2future_amd import _lib, back2future

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W = 128, 192
NAMES = {"hard": "random:hard:5:2.0", "soft": "random:soft:5:2.0"}
_models, _refs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()
    _refs.clear()


def model(which):
    if which not in _models:
        _models[which] = back2future.Model(NAMES[which])
    return _models[which]


def clip(seed, T, H0=H, W0=W, dtype=np.uint8):
    r = np.random.default_rng(seed)
    if dtype == np.uint8:
        return r.integers(0, 256, (T, 3, H0, W0), dtype=np.uint8)
    return r.random((T, 3, H0, W0), dtype=np.float32)


def reference(which, seed, T, H0=H, W0=W, dtype=np.uint8):
    """(frames, sequence outputs (flow, fwd, bwd, occ_prob)) of a clip: computed once, shared, never written."""
    key = (which, seed, T, H0, W0, np.dtype(dtype).name)
    if key not in _refs:
        V = clip(seed, T, H0, W0, dtype)
        out = model(which).computeFlowSequence(V, dtype=np.float32, occ_prob=True)
        for a in (V,) + tuple(out):
            a.setflags(write=False)
        _refs[key] = (V, out)
    return _refs[key]


def assert_push_equals(got, exp, i, what):
    assert got is not None, "%s: push %d returned None" % (what, i + 3)
    for j, (a, b) in enumerate(zip(got, exp)):
        np.testing.assert_array_equal(a[0], b[i], err_msg="%s: push %d, output %d" % (what, i + 3, j))


def run_stream(st, V, exp, what, between=None):
    for k in range(V.shape[0]):
        got = st.push(V[k], occ_prob=True)
        if k < 2:
            assert got is None, "%s: push %d is not ready" % (what, k + 1)
        else:
            assert_push_equals(got, exp, k - 2, what)
        if between:
            between()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_stream_equals_the_sequence(which, dtype):
    V, exp = reference(which, 1, 8, dtype=dtype)
    with model(which).openStream(H, W, dtype=dtype) as st:
        # pushes 1 and 2 write nothing into the caller's buffers
        out = (np.full((1, 2, H, W), 7.5, np.float32), np.full((1, 1, H, W), 9, np.uint8), np.full((1, 1, H, W), 9, np.uint8),
               np.full((1, 2, H, W), 7.5, np.float32))
        for k in range(2):
            assert st.push(V[k], out=out, occ_prob=True) is None
            assert all((a == (9 if a.dtype == np.uint8 else 7.5)).all() for a in out)
        for k in range(2, 8):
            got = st.push(V[k], out=out, occ_prob=True)
            assert got is not None and all(g is o for g, o in zip(got, out))
            assert_push_equals(got, exp, k - 2, "%s %s" % (which, np.dtype(dtype).name))
        assert st.frames_pushed == 8


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_stream_of_a_rescaled_size(which, dtype):
    V, exp = reference(which, 2, 6, 136, 200, dtype=dtype)
    with model(which).openStream(136, 200, dtype=dtype) as st:
        run_stream(st, V, exp, "%s 136x200 %s" % (which, np.dtype(dtype).name))


@pytest.mark.parametrize("H0,W0", [(H, W), (136, 200)])
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_device_push_equals_host_push(which, H0, W0):
    m = model(which)
    V, exp = reference(which, 3 if H0 == H else 2, 6, H0, W0)
    d = torch.from_numpy(V.copy()).cuda()
    flow = torch.full((1, 2, H0, W0), 7.5, device="cuda")
    prob = torch.empty((1, 2, H0, W0), device="cuda")
    fo = torch.empty((1, 1, H0, W0), dtype=torch.uint8, device="cuda")
    bo = torch.empty_like(fo)
    rgb = torch.empty((1, 3, H0, W0), dtype=torch.uint8, device="cuda")
    mx = torch.empty((1,), dtype=torch.float64, device="cuda")
    with m.openStream(H0, W0) as sd, m.openStream(H0, W0) as sh:
        for k in range(6):
            ready = sd.pushDevice(d[k].data_ptr(), flow.data_ptr(), prob.data_ptr(), fo.data_ptr(), bo.data_ptr())
            if ready:
                m.flowRGBDevice(flow.data_ptr(), 1, H0, W0, rgb.data_ptr(), d_max_used=mx.data_ptr())
            m.synchronize()
            pic = sh.pushRGB(V[k], want_flow=True)
            assert ready == (k >= 2) and (pic is not None) == ready
            if not ready:
                assert float(flow.min()) == 7.5 == float(flow.max())
                continue
            for j, t in enumerate((flow, fo, bo, prob)):
                np.testing.assert_array_equal(t.cpu().numpy()[0], exp[j][k - 2], err_msg="device push %d, output %d" % (k + 1, j))
            np.testing.assert_array_equal(rgb.cpu().numpy(), pic[0])
            np.testing.assert_array_equal(mx.cpu().numpy(), pic[1])
            np.testing.assert_array_equal(pic[2][0], exp[0][k - 2])


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_two_cameras(which):
    (Va, ea), (Vb, eb) = reference(which, 1, 8), reference(which, 4, 8)
    with model(which).openStream(H, W, cams=2) as st:
        for k in range(8):
            got = st.push(np.stack([Va[k], Vb[k]]), occ_prob=True)
            if k < 2:
                assert got is None
                continue
            for j in range(4):
                np.testing.assert_array_equal(got[j][0], ea[j][k - 2], err_msg="camera 0, push %d, output %d" % (k + 1, j))
                np.testing.assert_array_equal(got[j][1], eb[j][k - 2], err_msg="camera 1, push %d, output %d" % (k + 1, j))


def test_reset_starts_a_new_clip():
    (Va, _), (Vb, eb) = reference("hard", 1, 8), reference("hard", 4, 8)
    with model("hard").openStream(H, W) as st:
        for k in range(4):
            st.push(Va[k])
        assert st.frames_pushed == 4
        st.reset()
        assert st.frames_pushed == 0
        run_stream(st, Vb[:6], eb, "after reset")
        assert st.frames_pushed == 6


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_other_work_between_pushes(which):
    """computeFlowBatch at a larger size between every two pushes regrows the arena and the pipeline's buffers: the stream's state is its own."""
    m = back2future.Model(NAMES[which])   # a fresh context: the first batch call really grows the arena under the stream
    try:
        V, exp = reference(which, 1, 8)
        big = clip(9, 5, 192, 256)
        with m.openStream(H, W) as st:
            run_stream(st, V, exp, "%s with batches in between" % which,
                       between=lambda: m.computeFlowBatch(big[:3], big[1:4], big[2:5], dtype=np.float32))
    finally:
        m.close()


def test_two_streams_on_one_context():
    m = model("soft")
    (Va, ea), (Vb, eb) = reference("soft", 1, 8), reference("soft", 2, 6, 136, 200)
    with m.openStream(H, W) as sa, m.openStream(136, 200) as sb:
        for k in range(8):
            ga = sa.push(Va[k], occ_prob=True)
            gb = sb.push(Vb[k], occ_prob=True) if k < 6 else None
            if k >= 2:
                assert_push_equals(ga, ea, k - 2, "stream a")
                if k < 6:
                    assert_push_equals(gb, eb, k - 2, "stream b")


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_graph_replay(which):
    """use_graph = 1, device pushes: with T = 12 every ring phase goes through eager, capture and replay; then a new stream of the same
    shape (very likely at the same addresses) must not replay a graph of the closed one."""
    m = model(which)
    V, exp = reference(which, 5, 12)
    d = torch.from_numpy(V.copy()).cuda()
    outs = [torch.empty((1, 2, H, W), device="cuda"), torch.empty((1, 1, H, W), dtype=torch.uint8, device="cuda"),
            torch.empty((1, 1, H, W), dtype=torch.uint8, device="cuda"), torch.empty((1, 2, H, W), device="cuda")]
    with m.options(use_graph=1):
        for rnd in range(2):
            with m.openStream(H, W) as st:
                for k in range(12):
                    ready = st.pushDevice(d[k].data_ptr(), outs[0].data_ptr(), outs[3].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
                    m.synchronize()
                    assert ready == (k >= 2)
                    for j in range(4 if ready else 0):
                        np.testing.assert_array_equal(outs[j].cpu().numpy()[0], exp[j][k - 2], err_msg="round %d, push %d, output %d" % (rnd, k + 1, j))
    # host pushes replay graphs by default (host_graph = 1): T = 12 again
    with m.openStream(H, W) as st:
        run_stream(st, V, exp, "%s host graphs" % which)


@pytest.mark.parametrize("H0,W0,T", [(H, W, 8), (256, 384, 5)])
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_latency_rule_is_within_the_end_to_end_bar(which, H0, W0, T):
    """adaptive_kernels = 1: the per-launch rule may pick other kernels than the sequence did; the guarantee is DESIGN section 5's
    bar, max |d| <= 1e-3 on the flow (and on occ_prob).  At 128 x 192 both rules choose the same kernels for every launch; at
    256 x 384 the level-3 maps (64 x 96 = 6144 px >= wino4_min_pixels) run F(4x4) under the map-size rule and, one image being 12
    F(4x4) blocks against 48 F(2x2) blocks on 256 CUs, F(2x2) under the per-launch rule."""
    m = model(which)
    V, exp = reference(which, 6, T, H0, W0)
    worst = [0.0, 0.0]
    with m.options(adaptive_kernels=1):
        with m.openStream(H0, W0) as st:
            for k in range(T):
                got = st.push(V[k], occ_prob=True)
                if k >= 2:
                    worst[0] = max(worst[0], float(np.abs(got[0][0] - exp[0][k - 2]).max()))
                    worst[1] = max(worst[1], float(np.abs(got[3][0] - exp[3][k - 2]).max()))
    print("adaptive_kernels=1 vs default rule, %s %dx%d: max |d flow| = %.3g, max |d occ_prob| = %.3g (flow absmax %.3g)"
          % (which, H0, W0, worst[0], worst[1], float(np.abs(exp[0]).max())))
    assert worst[0] <= 1e-3 and worst[1] <= 1e-3, worst


@pytest.mark.parametrize("max_norm", [None, 20])
def test_push_rgb_equals_the_sequence_pictures(max_norm):
    m = model("soft")
    V, _ = reference("soft", 1, 8)
    for packed in (False, True):
        rgb, mx = m.computeFlowSequenceRGB(V, max=max_norm, packed=packed)
        with m.openStream(H, W) as st:
            for k in range(8):
                got = st.pushRGB(V[k], max=max_norm, packed=packed)
                if k < 2:
                    assert got is None
                    continue
                np.testing.assert_array_equal(got[0][0], rgb[k - 2])
                np.testing.assert_array_equal(got[1][0], mx[k - 2])


def test_errors_leave_the_stream_as_it_was():
    m = model("hard")
    V, exp = reference("hard", 1, 8)
    d = torch.from_numpy(V[:1].copy()).cuda()
    dflow = torch.empty((1, 2, H, W), device="cuda")
    hflow = np.empty((1, 2, H, W), np.float32)
    ready = C.c_int()
    L = _lib.lib()
    with m.openStream(H, W) as st:
        for k in range(3):
            st.push(V[k])
        bad = [
            (ValueError, "expected", lambda: st.push(np.zeros((3, H, W + 64), np.uint8))),
            (ValueError, "uint8 frames", lambda: st.push(np.zeros((3, H, W), np.float32))),
            (_lib.B2FError, "device memory", lambda: _lib.check(L.b2f_stream_push(st._h, C.c_void_p(d.data_ptr()), _lib.fptr(hflow), None, None, None,
                                                                                 C.byref(ready)))),
            (_lib.B2FError, "host memory", lambda: st.pushDevice(V[3].ctypes.data, dflow.data_ptr())),
            (_lib.B2FError, "host memory", lambda: st.pushDevice(d.data_ptr(), hflow.ctypes.data)),
            (_lib.B2FError, "16-byte aligned", lambda: st.pushDevice(d.data_ptr(), dflow.data_ptr() + 4)),
            (_lib.B2FError, "null argument", lambda: _lib.check(L.b2f_stream_push(st._h, C.c_void_p(V[3].ctypes.data), None, None, None, None,
                                                                                 C.byref(ready)))),
        ]
        for exc, match, call in bad:
            with pytest.raises(exc, match=match):
                call()
            assert st.frames_pushed == 3
        for k in range(3, 6):
            assert_push_equals(st.push(V[k], occ_prob=True), exp, k - 2, "after the refused pushes")
        # a failure inside a push: the stream is broken until reset
        m.set_option("debug_fail_next", 1)
        with pytest.raises(_lib.B2FError, match="forced failure"):
            st.push(V[6])
        with pytest.raises(_lib.B2FError, match="broken"):
            st.push(V[6])
        with pytest.raises(_lib.B2FError, match="broken"):
            st.pushDevice(d.data_ptr(), dflow.data_ptr())
        st.reset()
        run_stream(st, V[:4], exp, "after reset of a broken stream")
    with pytest.raises(ValueError, match="closed"):
        st.push(V[0])
    g = back2future.Model("random:hard", graph="win=5,levels=4")
    try:
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            g.openStream(H, W)
    finally:
        g.close()


def test_model_close_closes_its_streams():
    m = back2future.Model(NAMES["soft"])
    st = m.openStream(H, W)
    st.push(clip(0, 1)[0])
    m.close()
    assert st._h is None
    st.close()
