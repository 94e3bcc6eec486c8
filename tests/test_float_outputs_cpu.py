"""CPU: the float32 computeFlow entry points (b2f_compute_flow_batch_f32, b2f_compute_flow_sequence_f32, their b2f_multi forms and
the device entries b2f_compute_flow_device / b2f_compute_flow_sequence_device) are declared, exported and bound; they refuse
malformed arguments with a message before any HIP call; the Python keywords (dtype=, occ_prob=, out=) are validated before any
library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, flow_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["b2f_compute_flow_batch_f32", "b2f_compute_flow_sequence_f32", "b2f_multi_compute_flow_batch_f32",
         "b2f_multi_compute_flow_sequence_f32", "b2f_compute_flow_device", "b2f_compute_flow_sequence_device"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def test_the_six_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "b2f.h")).read()
    L = C.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert re.search(r"B2F_API\s+int\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, lua), "lua cdef lacks " + n
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n + "(" in doc, "INTEGRATION.md does not quote " + n


H, W = 64, 64
F = np.zeros((3, 3, H, W), np.float32)
FLOW = np.zeros((1, 2, H, W), np.float32)
OCC = np.zeros((1, 2, H, W), np.float32)
M1, M2 = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8)
_vp = lambda a: C.c_void_p(a.ctypes.data)
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))


def _call(name, ctx=None, count=None, in_kind=1, frames=F, h=H, w=W, flow=FLOW):
    """One call of `name` with every other argument valid; `count` = n (batch) or T (sequence)."""
    L = _lib.lib()
    seq = "sequence" in name
    count = (3 if seq else 1) if count is None else count
    fl = _lib.fptr(flow) if flow is not None else None
    ins = [_vp(frames)] if seq else [_vp(frames), _vp(frames), _vp(frames)]
    args = [ctx, count, in_kind] + ins + [h, w]
    if name.endswith("_device"):
        return getattr(L, name)(*args, C.c_void_p(flow.ctypes.data) if flow is not None else None, _vp(OCC), _vp(M1), _vp(M2), None)
    return getattr(L, name)(*args, fl, _lib.fptr(OCC), _up(M1), _up(M2))


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_fail_with_a_message_before_any_hip_call(name):
    """No GPU here: a HIP call would fail with a HIP error, so each message below shows the check came first."""
    seq = "sequence" in name
    cases = [
        (dict(), "null context"),
        (dict(flow=None), "null argument"),
        (dict(in_kind=back2future.IN_NORMALIZED), "B2F_IN_NORMALIZED is refused"),
        (dict(in_kind=7), "in_kind must be"),
        (dict(h=0), "bad shape"),
        (dict(w=-5), "bad shape"),
        (dict(h=32), "smaller than 64"),
        (dict(count=0), "T >= 3" if seq else "bad shape"),
    ]
    if seq:
        cases.append((dict(count=2), "T >= 3"))
    for kw, msg in cases:
        rc = _call(name, **kw)
        assert rc != 0, (name, kw)
        err = _lib.lib().b2f_last_error().decode()
        assert name in err and msg in err, (name, kw, err)


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
def test_keywords_validate_before_calling_the_library(cls, no_library):
    m = cls()
    a = np.zeros((2, 3, H, W), np.float32)
    V = np.zeros((4, 3, H, W), np.uint8)
    with pytest.raises(ValueError, match="occ_prob=True needs dtype=np.float32"):
        m.computeFlowBatch(a, a, a, occ_prob=True)
    with pytest.raises(ValueError, match="occ_prob=True needs dtype=np.float32"):
        m.computeFlowSequence(V, dtype=np.float64, occ_prob=True)
    for bad in (np.int32, np.float16, "complex64"):
        with pytest.raises(ValueError, match="dtype must be"):
            m.computeFlowBatch(a, a, a, dtype=bad)
        with pytest.raises(ValueError, match="dtype must be"):
            m.computeFlowSequence(V, dtype=bad)
    # out= must match the float32 outputs: dtype, shape, contiguity, and one buffer more with occ_prob
    good = (np.empty((2, 2, H, W), np.float32), np.empty((2, 1, H, W), np.uint8), np.empty((2, 1, H, W), np.uint8))
    bad_outs = [
        (np.empty((2, 2, H, W), np.float64),) + good[1:],
        (np.empty((2, 2, H, W + 1), np.float32),) + good[1:],
        (np.empty((2, 2, H, 2 * W), np.float32)[..., ::2],) + good[1:],
        good[:2],
    ]
    for out in bad_outs:
        with pytest.raises(ValueError, match="out"):
            m.computeFlowBatch(a, a, a, dtype=np.float32, out=out)
    with pytest.raises(ValueError, match="out must be"):
        m.computeFlowBatch(a, a, a, dtype=np.float32, occ_prob=True, out=good)
    with pytest.raises(ValueError, match=r"out\[3\]"):
        m.computeFlowBatch(a, a, a, dtype=np.float32, occ_prob=True, out=good + (np.empty((2, 1, H, W), np.float32),))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        m.computeFlowSequence(V, dtype=np.float32, out=(np.empty((3, 2, H, W), np.float32),) + good[1:])
    with pytest.raises(ValueError, match="T >= 3"):
        m.computeFlowSequence(V[:2], dtype=np.float32)
    if cls is _NoLib:
        with pytest.raises(ValueError, match="T >= 3"):
            m.computeFlowSequenceDevice(1 << 20, 2, H, W, 1 << 21)


def test_output_dtype_defaults_to_float64():
    assert back2future.output_dtype(np.float64, False, "x") == np.float64
    assert back2future.output_dtype("float32", True, "x") == np.float32


def test_writeflo_bytes_of_rounded_f64_equal_those_of_f32(tmp_path):
    """examples/run_sequence.py moved to the f32 entry: the .flo of np.float32(flow_f64) -- what it wrote before -- and the .flo
    of the f32 flow (which is np.float32(flow_f64) bit for bit) are the same file."""
    r = np.random.default_rng(3)
    f64 = r.standard_normal((2, 37, 53)) * 7.3
    f32 = np.float32(f64)
    flow_io.writeFLO(str(tmp_path / "a.flo"), f64.astype("float32"))
    flow_io.writeFLO(str(tmp_path / "b.flo"), f32)
    assert (tmp_path / "a.flo").read_bytes() == (tmp_path / "b.flo").read_bytes()
