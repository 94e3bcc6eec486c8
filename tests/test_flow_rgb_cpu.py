"""CPU: flow pictures (xy2rgb as a computeFlow output).  The seven entry points and the layout enum are declared, exported and bound; the host
entry b2f_flow_rgb_host reproduces the quantised flow_io.xy2rgb (the repo's restatement of flowExtensions.lua:17-150); every entry
refuses malformed arguments with a message before any HIP call; the Python wrappers validate before any library call.

Bounds against the yardstick: no byte may differ by more than 1 level, and at most 1e-6 of the bytes may differ at all.  The second
is a condition, not a courtesy: the yardstick with every angle moved by +-1 ulp (a different atan) stays at 0 differing bytes, an
fp32 implementation lands at 1.2e-5 .. 2.0e-5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, flow_io, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["b2f_flow_rgb_host", "b2f_flow_rgb_device", "b2f_op_flow_rgb", "b2f_compute_flow_batch_rgb", "b2f_compute_flow_sequence_rgb",
         "b2f_multi_compute_flow_batch_rgb", "b2f_multi_compute_flow_sequence_rgb"]
ENUMS = ["B2F_RGB_PLANAR", "B2F_RGB_PACKED"]
MAX_LEVELS = 1
MAX_SHARE = 1e-6


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
    for e in ENUMS:
        assert e in src and e in lua and e in doc, e
    assert (back2future.RGB_PLANAR, back2future.RGB_PACKED) == (0, 1)
    assert L.b2f_version() >= 1001


def quantise(rgb):
    """flow_io.save_image's bytes: floor(clip(v, 0, 1) * 255 + 0.5)"""
    return (np.clip(np.asarray(rgb, np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def field_a(H=1024, W=1920, seed=0):
    """Sines up to 30 px plus noise, with rows of exact x == 0, y == 0 and zero flow."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    x = (30 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + rng.normal(0, 2, (H, W))).astype(np.float32)
    y = (12 * np.cos(xx / 45.0) + rng.normal(0, 2, (H, W))).astype(np.float32)
    x[:8] = 0
    y[8:16] = 0
    x[16:20] = 0
    y[16:20] = 0
    return np.stack([x, y])


def yardstick(flow, max=None):
    """(planar bytes, max) of flow_io.xy2rgb on a 2 x H x W field"""
    rgb, mx = flow_io.xy2rgb(flow[0], flow[1], max)
    return quantise(rgb), mx


def compare(got, want, what):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    levels, differing = int(d.max()), int((d > 0).sum())
    print("%s: largest byte difference %d, %d of %d bytes differ (%.2e)" % (what, levels, differing, d.size, differing / d.size))
    assert levels <= MAX_LEVELS, what
    assert differing <= MAX_SHARE * d.size, what


@pytest.fixture(scope="module")
def field():
    return field_a()


@pytest.mark.parametrize("max", [None, 20.0])
def test_field_a_matches_the_yardstick(field, max):
    want, mx = yardstick(field, max)
    for packed in (False, True):
        rgb, used = ops.flow_rgb(field, max=max, packed=packed)
        assert rgb.dtype == np.uint8 and rgb.shape == ((1024, 1920, 3) if packed else (3, 1024, 1920))
        compare(rgb.transpose(2, 0, 1) if packed else rgb, want, "field A, max=%r, packed=%r" % (max, packed))
        assert used.dtype == np.float64 and used.shape == (1,)
        assert used[0] == mx
    if max is None:
        norm = flow_io.computeNorm(field[0], field[1])
        assert used[0].tobytes() == np.float64(builtins_max(float(norm.max()), 1e-2)).tobytes()


def builtins_max(a, b):
    return a if a > b else b


def test_zero_flow_is_white():
    for max in (None, 3.0):
        rgb, used = ops.flow_rgb(np.zeros((2, 5, 7), np.float32), max=max)
        assert (rgb == 255).all()
        assert used[0] == (1e-2 if max is None else 3.0)


def test_axes_and_diagonals_at_full_saturation():
    """The four axis directions and the four diagonals, each the largest flow of its own image, so s = 1."""
    r = np.float32(2.5)
    dirs = [(r, 0), (0, r), (-r, 0), (0, -r), (r, r), (-r, r), (-r, -r), (r, -r)]
    flow = np.zeros((len(dirs), 2, 1, 2), np.float32)   # pixel 0 carries the direction, pixel 1 is null flow
    for i, (x, y) in enumerate(dirs):
        flow[i, 0, 0, 0], flow[i, 1, 0, 0] = x, y
    rgb, used = ops.flow_rgb(flow)
    for i in range(len(dirs)):
        want, mx = yardstick(flow[i])
        assert (rgb[i] == want).all(), (dirs[i], rgb[i].ravel(), want.ravel())
        assert used[i] == mx
        assert tuple(rgb[i][:, 0, 1]) == (255, 255, 255)
    # pure hues at s = 1, l = 1/2: +x is red (0 degrees), -x is cyan (180 degrees)
    assert tuple(rgb[0][:, 0, 0]) == (255, 0, 0) and tuple(rgb[2][:, 0, 0]) == (0, 255, 255)
    # with a caller-given maximum the saturation is tanh'ed
    rgb, used = ops.flow_rgb(flow, max=2.5)
    for i in range(len(dirs)):
        assert (rgb[i] == yardstick(flow[i], 2.5)[0]).all()
        assert used[i] == 2.5


def test_small_norms_are_divided_by_a_hundredth():
    rng = np.random.default_rng(1)
    flow = (rng.normal(0, 1e-3, (2, 3, 5))).astype(np.float32)
    assert float(flow_io.computeNorm(flow[0], flow[1]).max()) < 1e-2
    rgb, used = ops.flow_rgb(flow)
    assert used[0] == 1e-2
    assert (rgb == yardstick(flow)[0]).all()
    rgb, used = ops.flow_rgb(flow, max=1e-3)   # a caller-given maximum below 1e-2 too
    assert used[0] == 1e-2
    assert (rgb == yardstick(flow, 1e-3)[0]).all()


def test_every_image_gets_its_own_maximum():
    rng = np.random.default_rng(2)
    flow = rng.normal(0, 1, (3, 2, 3, 5)).astype(np.float32) * np.array([0.5, 4.0, 40.0], np.float32)[:, None, None, None]
    rgb, used = ops.flow_rgb(flow)
    assert len(set(used.tolist())) == 3
    for i in range(3):
        want, mx = yardstick(flow[i])
        assert used[i] == mx
        assert (rgb[i] == want).all()


@pytest.mark.parametrize("shape", [(1, 1), (3, 5)])
@pytest.mark.parametrize("max", [None, 1.5])
def test_tiny_images_and_packed_is_planar_transposed(shape, max):
    rng = np.random.default_rng(3)
    flow = rng.normal(0, 2, (2, 2) + shape).astype(np.float32)
    planar, used = ops.flow_rgb(flow, max=max)
    packed, used_p = ops.flow_rgb(flow, max=max, packed=True)
    assert planar.shape == (2, 3) + shape and packed.shape == (2,) + shape + (3,)
    assert (packed == planar.transpose(0, 2, 3, 1)).all() and (used == used_p).all()
    for i in range(2):
        assert (planar[i] == yardstick(flow[i], max)[0]).all()
    one, _ = ops.flow_rgb(flow[0], max=max)   # 2 x H x W in, 3 x H x W out
    assert one.shape == (3,) + shape and (one == planar[0]).all()


# ---- argument checks: before any HIP call (no GPU here: a HIP call would fail with a HIP error instead) ----
H, W = 64, 64
FRAMES = np.zeros((3, 3, H, W), np.float32)
FLOW = np.zeros((1, 2, H, W), np.float32)
RGB = np.zeros((1, 3, H, W), np.uint8)
MX = np.zeros(1, np.float64)
M1, M2 = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8)
_vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _call(name, count=None, h=H, w=W, layout=0, rgb=RGB, flow=FLOW, offset=0):
    """One call of `name` with a null context and every other argument valid"""
    L = _lib.lib()
    fl = _lib.fptr(flow) if flow is not None else None
    if name == "b2f_flow_rgb_host":
        return L.b2f_flow_rgb_host(fl, 1 if count is None else count, h, w, 0.0, layout, _up(rgb), _dp(MX))
    if name == "b2f_op_flow_rgb":
        return L.b2f_op_flow_rgb(None, fl, 1 if count is None else count, h, w, 0.0, layout, _up(rgb), _dp(MX))
    if name == "b2f_flow_rgb_device":
        return L.b2f_flow_rgb_device(None, C.c_void_p(flow.ctypes.data + offset) if flow is not None else None, 1 if count is None else count,
                                     h, w, 0.0, layout, _vp(rgb), None, None)
    seq = "sequence" in name
    count = (3 if seq else 1) if count is None else count
    ins = [_vp(FRAMES)] if seq else [_vp(FRAMES)] * 3
    return getattr(L, name)(None, count, back2future.IN_UNIT, *ins, h, w, 0.0, layout, _up(rgb), _dp(MX), fl, _up(M1), _up(M2))


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_fail_with_a_message_before_any_hip_call(name):
    compute = "compute_flow" in name
    cases = [
        (dict(layout=2), "bad layout"),
        (dict(layout=-1), "bad layout"),
        (dict(h=0), "bad shape"),
        (dict(w=-5), "bad shape"),
        (dict(rgb=None), "null argument"),
    ]
    if "sequence" in name:
        cases += [(dict(count=2), "T >= 3"), (dict(count=0), "T >= 3")]
    else:
        cases.append((dict(count=0), "bad shape"))
    if not compute:
        cases.append((dict(flow=None), "null argument"))   # the computeFlow forms may leave the flow out
    if name != "b2f_flow_rgb_host":
        cases.append((dict(), "null context"))
    for kw, msg in cases:
        rc = _call(name, **kw)
        assert rc != 0, (name, kw)
        err = _lib.lib().b2f_last_error().decode()
        assert name in err and msg in err, (name, kw, err)
    if compute:   # without the flow the request is still complete: the first complaint is the context
        assert _call(name, flow=None) != 0
        assert "null context" in _lib.lib().b2f_last_error().decode()


def test_the_device_entry_refuses_misaligned_pointers():
    """The alignment is a check of the pointer values: a base offset by 4 bytes is refused whatever else is passed"""
    assert _call("b2f_flow_rgb_device", offset=4) != 0
    err = _lib.lib().b2f_last_error().decode()
    assert "b2f_flow_rgb_device" in err and "16-byte aligned" in err, err
    assert _call("b2f_flow_rgb_device", offset=16) != 0
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
    a = np.zeros((2, 3, H, W), np.float32)
    V = np.zeros((4, 3, H, W), np.uint8)
    for bad in (0, -1.0, float("nan"), "big"):
        with pytest.raises(ValueError, match="max must be"):
            m.computeFlowBatchRGB(a, a, a, max=bad)
        with pytest.raises(ValueError, match="max must be"):
            m.computeFlowSequenceRGB(V, max=bad)
    with pytest.raises(ValueError, match="n x 3 x H x W"):
        m.computeFlowBatchRGB(a, a, a[:1])
    with pytest.raises(ValueError, match="n x 3 x H x W"):
        m.computeFlowBatchRGB(a[0], a[0], a[0])
    with pytest.raises(ValueError, match="n x 3 x H x W"):
        m.computeFlowBatchRGB(a[:, :2], a[:, :2], a[:, :2])
    with pytest.raises(ValueError, match="T >= 3"):
        m.computeFlowSequenceRGB(V[:2])
    with pytest.raises(ValueError, match="T x 3 x H x W"):
        m.computeFlowSequenceRGB(V[:, :2])
    # out= must be the returned tuple's buffers
    good = (np.empty((2, 3, H, W), np.uint8), np.empty(2, np.float64))
    with pytest.raises(ValueError, match="out must be"):
        m.computeFlowBatchRGB(a, a, a, want_flow=True, out=good)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        m.computeFlowBatchRGB(a, a, a, packed=True, out=good)
    with pytest.raises(ValueError, match=r"out\[1\]"):
        m.computeFlowSequenceRGB(V, out=(good[0], np.empty(2, np.float32)))


def test_flow_rgb_and_the_device_wrapper_validate_before_calling_the_library(no_library):
    for bad in (np.zeros((3, 4, 4), np.float32), np.zeros((2, 3, 4, 4), np.float32), np.zeros((4, 4), np.float32),
                np.zeros((0, 2, 4, 4), np.float32), np.zeros((2, 0, 4), np.float32)):
        with pytest.raises(ValueError, match="flow_rgb: expected"):
            ops.flow_rgb(bad)
    with pytest.raises(ValueError, match="max must be"):
        ops.flow_rgb(np.zeros((2, 4, 4), np.float32), max=0)
    m = _NoLib()
    with pytest.raises(ValueError, match="max must be"):
        m.flowRGBDevice(4096, 1, 4, 4, 8192, max=-2)
    with pytest.raises(ValueError, match="bad shape"):
        m.flowRGBDevice(4096, 0, 4, 4, 8192)
