"""GPU: motion compensation and the past flow per pushed frame (Model.openStream(warp=, past=), MotionStream.pushWarp / pushPast /
pushDeviceWarp; b2f_stream_open_ex, b2f_stream_push_warp*, b2f_stream_push_past*).  The stage is the sequence entries' own
(flow_warp_kernel on the stream's kept frames, outputs_f32_kernel on the past-flow planes), so push k >= 3 must be output k - 3 of
computeFlowSequenceWarp / computeFlowSequencePast on the same frames bit for bit, in every output; and, so that a mistake the two
paths share cannot hide, the host definition (ops.flow_warp(model=None)) of the flow and occ_prob a push returned and the caller's own
three frames must give the push's warped frames and photometric words exactly.

Sizes: 128 x 192 (a /64 size: the frame slots hold the caller's frames) and 136 x 200 (rescaled: the raw ring does).  T = 7 frames, so
every ring slot is reused.  tests/test_stream_warp_cpu.py shows that these clips tell the slots apart."""
import ctypes as C

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import stream_warp_clips as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = {"hard": "random:hard:5:2.0", "soft": "random:soft:5:2.0"}   # as tests/test_gpu_stream.py opens them
T = SC.T
SA, SB = SC.SEEDS
ALL = dict(want_flow=True, want_masks=True, want_prob=True)
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


def reference(which, seed, H0, W0, dtype=np.uint8, own=False):
    """(frames, computeFlowSequenceWarp's (warped, photo, flow, fwd_occ, bwd_occ, occ_prob[, past_flow])): computed once, shared, never
    written"""
    key = (which, seed, H0, W0, np.dtype(dtype).name, own)
    if key not in _refs:
        V = SC.clip(seed, H0, W0, dtype)
        out = model(which).computeFlowSequenceWarp(V, own_past_flow=own, want_past=own, **ALL)
        for a in (V,) + tuple(out):
            a.setflags(write=False)
        _refs[key] = (V, out)
    return _refs[key]


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
        raise AssertionError("%s: %d of %d values differ" % (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()), a.size))


def assert_push(got, exp, i, what, cam=0):
    """the outputs of a push (leading cams axis) against element i of the sequence's"""
    assert got is not None, "%s: push %d returned None" % (what, i + 3)
    assert len(got) == len(exp), what
    for j, (a, b) in enumerate(zip(got, exp)):
        _eq(a[cam], b[i], "%s: push %d, output %d" % (what, i + 3, j))


def assert_host_definition(got, V, k, what, past=None):
    """ops.flow_warp(model=None) of the push's own flow and occ_prob and the caller's frames (k - 2, k - 1, k) gives its warped, photo"""
    warped, photo, flow, _, _, prob = got[:6]
    w, p = ops.flow_warp(flow, V[k - 2][None], V[k - 1][None], V[k][None], occ_prob=prob, model=None, own_past_flow=past is not None,
                         past_flow=past)
    _eq(warped, w, "%s: push %d, warped frames against the host definition" % (what, k + 1))
    _eq(photo, p, "%s: push %d, photo words against the host definition" % (what, k + 1))


# ---- 1, 2: a push equals the sequence and the host definition ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("H0,W0", SC.SIZES)
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_push_equals_the_sequence_and_the_host_definition(which, H0, W0, dtype):
    V, exp = reference(which, SA, H0, W0, dtype)
    what = "%s %dx%d %s" % (which, H0, W0, np.dtype(dtype).name)
    with model(which).openStream(H0, W0, dtype=dtype, warp=True) as st:
        for k in range(T):
            got = st.pushWarp(V[k], **ALL)
            if k < 2:
                assert got is None, "%s: push %d is not ready" % (what, k + 1)
                continue
            assert got[0].dtype == dtype and got[0].shape == (1, 2, 3, H0, W0) and got[1].shape == (1, back2future.PHOTO_WORDS)
            assert_push(got, exp, k - 2, what)
            assert_host_definition(got, V, k, what)
        assert st.frames_pushed == T


def test_outputs_left_out_and_caller_buffers():
    """photo alone (112 bytes per camera come down) and warped alone, into the caller's buffers; pushes 1 and 2 write nothing"""
    H0, W0 = SC.SIZES[1]
    V, exp = reference("hard", SA, H0, W0)
    m = model("hard")
    photo = np.full((1, back2future.PHOTO_WORDS), 7, np.uint64)
    warped = np.full((1, 2, 3, H0, W0), 9, np.uint8)
    with m.openStream(H0, W0, warp=True) as sp, m.openStream(H0, W0, warp=True) as sw:
        for k in range(T):
            gp = sp.pushWarp(V[k], want_warped=False, out=photo)
            gw = sw.pushWarp(V[k], want_photo=False, out=warped)
            if k < 2:
                assert gp is None and gw is None and (photo == 7).all() and (warped == 9).all()
                continue
            assert gp is photo and gw is warped
            _eq(photo[0], exp[1][k - 2], "photo alone, push %d" % (k + 1))
            _eq(warped[0], exp[0][k - 2], "warped alone, push %d" % (k + 1))
        s = back2future.photo_summary(photo)
        assert s == back2future.photo_summary(exp[1][T - 3]) and s["nonfinite"] == 0


# ---- 3: the model's own past flow ----

@pytest.mark.parametrize("H0,W0", SC.SIZES)
def test_own_past_flow(H0, W0):
    V, exp = reference("soft", SA, H0, W0, own=True)
    m = model("soft")
    past_exp = m.computeFlowSequencePast(V, occ_prob=True)
    what = "soft %dx%d own past flow" % (H0, W0)
    with m.openStream(H0, W0, warp=True, past=True) as sw, m.openStream(H0, W0, past=True) as sp:
        for k in range(T):
            got = sw.pushWarp(V[k], own_past_flow=True, want_past=True, **ALL)
            gp = sp.pushPast(V[k], occ_prob=True)
            if k < 2:
                assert got is None and gp is None
                continue
            assert len(got) == 7
            assert_push(got, exp, k - 2, what)
            assert_host_definition(got, V, k, what, past=got[6])
            assert_push(gp, past_exp, k - 2, what + ", pushPast")
            _eq(gp[1], got[6], what + ": the past flow of both pushes")
    # without own_past_flow the stream's warp is the plain one, whatever it was opened with
    Vp, plain = reference("soft", SA, H0, W0)
    with m.openStream(H0, W0, warp=True, past=True) as st:
        for k in range(4):
            got = st.pushWarp(V[k], **ALL)
            if k >= 2:
                assert_push(got, plain, k - 2, what + ", plain warp push")


def test_a_hard_model_opens_no_past_stream():
    m = model("hard")
    for kw in (dict(past=True), dict(warp=True, past=True)):
        with pytest.raises(_lib.B2FError, match=r"this model has no past-flow decoders \(a Hard or two_frame model estimates the future flow only\)"):
            m.openStream(128, 192, **kw)
    H0, W0 = SC.SIZES[0]
    V, exp = reference("hard", SA, H0, W0)
    with m.openStream(H0, W0, warp=True) as st:    # the context works afterwards
        for k in range(3):
            got = st.pushWarp(V[k], **ALL)
        assert_push(got, exp, 0, "hard, after the refused opens")


# ---- 4: device pushes and graph replay ----

def _device_outputs(H0, W0, past):
    f = lambda *s: torch.full(s, 7.5, device="cuda")
    b = lambda *s: torch.full(s, 9, dtype=torch.uint8, device="cuda")
    return {"warped": b(1, 2, 3, H0, W0), "photo": torch.full((1, back2future.PHOTO_WORDS), 7, dtype=torch.int64, device="cuda"),
            "flow": f(1, 2, H0, W0), "fwd": b(1, 1, H0, W0), "bwd": b(1, 1, H0, W0), "prob": f(1, 2, H0, W0),
            "past": f(1, 2, H0, W0) if past else None}


def _device_push(st, d_frame, o, own):
    p = lambda t: t.data_ptr() if t is not None else None
    return st.pushDeviceWarp(d_frame.data_ptr(), d_warped=p(o["warped"]), d_photo=p(o["photo"]), d_flow=p(o["flow"]), d_occ_prob=p(o["prob"]),
                             d_fwd_occ=p(o["fwd"]), d_bwd_occ=p(o["bwd"]), own_past_flow=own, d_past_flow=p(o["past"]))


def _device_results(o):
    order = ["warped", "photo", "flow", "fwd", "bwd", "prob", "past"]
    return [o[n].cpu().numpy().view(np.uint64) if n == "photo" else o[n].cpu().numpy() for n in order if o[n] is not None]


@pytest.mark.parametrize("H0,W0", SC.SIZES)
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_device_push_equals_host_push(which, H0, W0):
    own = which == "soft"
    m = model(which)
    V, exp = reference(which, SA, H0, W0, own=own)
    d = torch.from_numpy(V.copy()).cuda()
    o = _device_outputs(H0, W0, own)
    what = "%s %dx%d device push" % (which, H0, W0)
    with m.openStream(H0, W0, warp=True, past=own) as st:
        for k in range(T):
            ready = _device_push(st, d[k], o, own)
            m.synchronize()
            assert ready == (k >= 2)
            if not ready:
                assert float(o["flow"].min()) == 7.5 and int(o["warped"].min()) == 9 and int(o["photo"].min()) == 7
                continue
            assert_push(_device_results(o), exp, k - 2, what)
    # the records alone: flow, occ_prob and the past flow stay in the stream's own buffers
    photo = torch.zeros((1, back2future.PHOTO_WORDS), dtype=torch.int64, device="cuda")
    with m.openStream(H0, W0, warp=True, past=own) as st:
        for k in range(4):
            ready = st.pushDeviceWarp(d[k].data_ptr(), d_photo=photo.data_ptr(), own_past_flow=own)
            m.synchronize()
            if ready:
                _eq(photo.cpu().numpy().view(np.uint64)[0], exp[1][k - 2], what + ", records alone, push %d" % (k + 1))


def test_device_past_push():
    H0, W0 = SC.SIZES[1]
    m = model("soft")
    V = SC.clip(SA, H0, W0, np.uint8)
    exp = m.computeFlowSequencePast(V[:4], occ_prob=True)
    d = torch.from_numpy(V.copy()).cuda()
    flow, past, prob = (torch.empty((1, 2, H0, W0), device="cuda") for _ in range(3))
    fo, bo = (torch.empty((1, 1, H0, W0), dtype=torch.uint8, device="cuda") for _ in range(2))
    with m.openStream(H0, W0, past=True) as st:
        for k in range(4):
            ready = st.pushDevicePast(d[k].data_ptr(), flow.data_ptr(), past.data_ptr(), prob.data_ptr(), fo.data_ptr(), bo.data_ptr())
            m.synchronize()
            assert ready == (k >= 2)
            if ready:
                assert_push([t.cpu().numpy() for t in (flow, past, fo, bo, prob)], exp, k - 2, "pushDevicePast")


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_graph_replay(which):
    """use_graph = 1, device pushes: three rounds of T = 7 pushes on one stream (a reset keeps its pointers, and so its graphs) take
    every ring phase through eager, capture and replay -- the phase of slot 1 is used once per round, at push 5.  Then the same with
    host pushes, which replay graphs by default (host_graph = 1)."""
    own = which == "soft"
    H0, W0 = SC.SIZES[1]
    m = model(which)
    V, exp = reference(which, SA, H0, W0, own=own)
    d = torch.from_numpy(V.copy()).cuda()
    o = _device_outputs(H0, W0, own)
    with m.options(use_graph=1):
        with m.openStream(H0, W0, warp=True, past=own) as st:
            for rnd in range(3):
                for k in range(T):
                    ready = _device_push(st, d[k], o, own)
                    m.synchronize()
                    if ready:
                        assert_push(_device_results(o), exp, k - 2, "%s replay round %d" % (which, rnd))
                st.reset()
    with m.openStream(H0, W0, warp=True, past=own) as st:
        for rnd in range(3):
            for k in range(T):
                got = st.pushWarp(V[k], own_past_flow=own, want_past=own, **ALL)
                if k >= 2:
                    assert_push(got, exp, k - 2, "%s host graphs round %d" % (which, rnd))
            st.reset()


# ---- 5: two cameras ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("H0,W0", SC.SIZES)
def test_two_cameras(H0, W0, dtype):
    (Va, ea), (Vb, eb) = reference("hard", SA, H0, W0, dtype), reference("hard", SB, H0, W0, dtype)
    with model("hard").openStream(H0, W0, cams=2, dtype=dtype, warp=True) as st:
        for k in range(T):
            got = st.pushWarp(np.stack([Va[k], Vb[k]]), **ALL)
            if k < 2:
                assert got is None
                continue
            assert_push(got, ea, k - 2, "camera 0", cam=0)
            assert_push(got, eb, k - 2, "camera 1", cam=1)


# ---- 6: plain and warp pushes on one stream; reset ----

@pytest.mark.parametrize("H0,W0", SC.SIZES)
@pytest.mark.parametrize("which", ["hard", "soft"])
def test_mixed_pushes_and_reset(which, H0, W0):
    (Va, ea), (Vb, eb) = reference(which, SA, H0, W0), reference(which, SB, H0, W0)
    plain = lambda e: (e[2], e[3], e[4], e[5])   # (flow, fwd_occ, bwd_occ, occ_prob) as push(occ_prob=True) returns them
    with model(which).openStream(H0, W0, warp=True) as st:
        for V, e, first in ((Va, ea, 0), (Vb, eb, 1)):
            for k in range(T):
                if (k + first) % 2:
                    got = st.push(V[k], occ_prob=True)
                    exp = plain(e)
                else:
                    got = st.pushWarp(V[k], **ALL)
                    exp = e
                if k < 2:
                    assert got is None
                else:
                    assert_push(got, exp, k - 2, "%s %dx%d mixed pushes" % (which, H0, W0))
            assert st.frames_pushed == T
            st.reset()
            assert st.frames_pushed == 0


# ---- 7: refusals leave the stream as it was ----

def test_refusals_leave_the_stream_as_it_was():
    H0, W0 = SC.SIZES[1]
    m = model("soft")
    V, exp = reference("soft", SA, H0, W0)
    plain = (exp[2], exp[3], exp[4], exp[5])
    L = _lib.lib()
    ready = C.c_int(5)
    photo = np.zeros((1, back2future.PHOTO_WORDS), np.uint64)
    flow = np.empty((1, 2, H0, W0), np.float32)
    with m.openStream(H0, W0, past=True) as st:   # opened without warp: the message names the flag
        for k in range(3):
            st.push(V[k])
        for kw in (dict(), dict(own_past_flow=True)):
            with pytest.raises(_lib.B2FError, match="B2F_STREAM_WARP"):
                st.pushWarp(V[3], **kw)
            assert st.frames_pushed == 3
        assert_push(st.push(V[3], occ_prob=True), plain, 1, "a stream opened without warp after the refused pushes")
    with m.openStream(H0, W0) as st:   # a plain stream: a FlowStream without these pushes; the library's entries refuse on it
        assert type(st) is back2future.FlowStream and not hasattr(st, "pushWarp") and not hasattr(st, "pushPast")
        for k in range(3):
            st.push(V[k])
        calls = [("B2F_STREAM_WARP", lambda: L.b2f_stream_push_warp(st._h, C.c_void_p(V[3].ctypes.data), 20.0, 0, None,
                                                                     photo.ctypes.data_as(C.POINTER(C.c_ulonglong)), None, None, None, None, None,
                                                                     C.byref(ready))),
                 ("B2F_STREAM_PAST", lambda: L.b2f_stream_push_past(st._h, C.c_void_p(V[3].ctypes.data), _lib.fptr(flow), _lib.fptr(flow), None, None,
                                                                     None, C.byref(ready)))]
        for match, call in calls:
            with pytest.raises(_lib.B2FError, match=match):
                _lib.check(call())
            assert st.frames_pushed == 3 and ready.value == 0
        assert_push(st.push(V[3], occ_prob=True), plain, 1, "a plain stream after the refused pushes")
    ready = C.c_int(5)
    with m.openStream(H0, W0, warp=True) as st:
        for k in range(3):
            st.pushWarp(V[k])
        bad = [
            ("at least one of warped and photo", lambda: _lib.check(L.b2f_stream_push_warp(st._h, C.c_void_p(V[3].ctypes.data), 20.0, 0, None, None,
                                                                                           _lib.fptr(flow), None, None, None, None, C.byref(ready)))),
            ("flow_scale must be finite and > 0", lambda: st.pushWarp(V[3], flow_scale=0.0)),
            ("flow_scale must be finite and > 0", lambda: st.pushWarp(V[3], flow_scale=-20.0)),
            ("flow_scale must be finite and > 0", lambda: st.pushWarp(V[3], flow_scale=float("nan"))),
            ("B2F_STREAM_PAST", lambda: st.pushWarp(V[3], own_past_flow=True)),
            ("B2F_STREAM_PAST", lambda: st.pushPast(V[3])),
        ]
        for match, call in bad:
            with pytest.raises(_lib.B2FError, match=match):
                call()
            assert st.frames_pushed == 3 and ready.value in (0, 5)
        with pytest.raises(ValueError, match="at least one of want_warped and want_photo"):
            st.pushWarp(V[3], want_warped=False, want_photo=False)
        assert st.frames_pushed == 3
        for k in range(3, T):
            assert_push(st.pushWarp(V[k], **ALL), exp, k - 2, "after the refused pushes")


# ---- 8: guards ----

@pytest.mark.parametrize("which", ["hard", "soft"])
def test_guarded_context(which):
    """arena_guard / arena_fill: the stream's block (raw ring and warp buffers included) starts as the NaN pattern; a clip of warp pushes
    leaves every guard word as it was and equals the plain context bit for bit"""
    own = which == "soft"
    H0, W0 = SC.SIZES[1]
    V, exp = reference(which, SA, H0, W0, own=own)
    g = back2future.Model(NAMES[which])
    try:
        g.set_option("arena_guard", 4096)
        g.set_option("arena_fill", 1)
        with g.openStream(H0, W0, warp=True, past=own) as st:
            for k in range(T):
                got = st.pushWarp(V[k], own_past_flow=own, want_past=own, **ALL)
                n, _, _, msg = g.arena_check(detail=True)
                assert n == 0, "push %d: %d guard words overwritten; %s" % (k + 1, n, msg)
                if k >= 2:
                    assert_push(got, exp, k - 2, "%s guarded" % which)
    finally:
        g.close()
