"""CPU: the stream entries for motion compensation and the past flow (b2f_stream_open_ex, b2f_stream_flags, b2f_stream_push_warp[_device],
b2f_stream_push_past[_device]) are declared, exported and bound with the header's argument counts, usable from C, and fail with a message
on a NULL stream; MotionStream.pushWarp / pushPast validate like their sequence counterparts before any library call; and the clips of
tests/test_gpu_stream_warp.py can tell the ring slots of a stream apart."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build
from tests import stream_warp_clips as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> arguments in include/b2f.h
ARGS = {"b2f_stream_open_ex": 7, "b2f_stream_flags": 2, "b2f_stream_push_warp": 12, "b2f_stream_push_warp_device": 13,
        "b2f_stream_push_past": 8, "b2f_stream_push_past_device": 9}


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def _header():
    return open(os.path.join(ROOT, "include", "b2f.h")).read()


def test_header_declares_the_entries_and_the_table_binds_them_with_the_same_argument_counts():
    src = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    L = C.CDLL(_lib.SO_PATH)
    for name, count in ARGS.items():
        m = re.search(r"B2F_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == count, name
        assert hasattr(L, name), name + " is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == count, name
    assert re.search(r"B2F_STREAM_WARP\s*=\s*1\b", src) and re.search(r"B2F_STREAM_PAST\s*=\s*2\b", src)
    assert (back2future.STREAM_WARP, back2future.STREAM_PAST) == (1, 2)


def test_every_entry_cites_what_it_mirrors():
    src = _header()
    part = src[src.index("streams with motion compensation"):src.index("b2f_stream_push_past_device(")]
    for cite in ("models/pwc.lua:67-73", "criterions/OBCCriterion.lua:79-100", "models/pwc.lua:328-385", "back2future.lua:54-71",
                 "b2f_compute_flow_sequence_warp", "b2f_compute_flow_sequence_warp_past", "b2f_compute_flow_sequence_past"):
        assert cite in part, cite
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ARGS:
        assert name + "(" in doc, "INTEGRATION.md does not quote " + name


C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "b2f.h"
int main(void)
{
    static unsigned char u[3 * 64 * 64], warped[6 * 64 * 64];
    static float flow[2 * 64 * 64];
    unsigned long long photo[B2F_PHOTO_WORDS];
    b2f_stream *st = (b2f_stream *)u;
    int ready = 5, flags = 7, rc;
    rc = b2f_stream_open_ex(NULL, 1, B2F_IN_U8, 64, 64, B2F_STREAM_WARP | B2F_STREAM_PAST, &st);
    if (st != NULL || strstr(b2f_last_error(), "b2f_stream_open_ex: null context") == NULL) return 2;
    rc += b2f_stream_push_warp(NULL, u, 20.0, 0, warped, photo, NULL, NULL, NULL, NULL, NULL, &ready);
    if (strstr(b2f_last_error(), "b2f_stream_push_warp: null stream") == NULL) return 3;
    rc += b2f_stream_push_warp_device(NULL, u, 20.0, 1, warped, photo, flow, NULL, NULL, NULL, flow, NULL, &ready);
    if (strstr(b2f_last_error(), "b2f_stream_push_warp_device: null stream") == NULL) return 4;
    rc += b2f_stream_push_past(NULL, u, flow, flow, NULL, NULL, NULL, &ready);
    if (strstr(b2f_last_error(), "b2f_stream_push_past: null stream") == NULL) return 5;
    rc += b2f_stream_push_past_device(NULL, u, flow, flow, NULL, NULL, NULL, NULL, &ready);
    rc += b2f_stream_flags(NULL, &flags);
    if (flags != 7 || ready != 5) return 6;
    printf("%d %s\n", rc, b2f_last_error());
    return rc == 6 ? 0 : 1;
}
"""


def test_c99_program_gets_the_text_not_a_crash(tmp_path):
    src = tmp_path / "stream_warp.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "stream_warp")
    lib_dir = os.path.join(ROOT, "back2future_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", exe, "-L" + lib_dir, "-lb2f", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "b2f_stream_flags: null stream" in r.stdout


def test_entries_fail_loudly_from_python_too():
    L = _lib.lib()
    u = np.zeros((1, 3, 64, 64), np.uint8)
    w = np.zeros((1, 2, 3, 64, 64), np.uint8)
    photo = np.zeros((1, back2future.PHOTO_WORDS), np.uint64)
    flow = np.zeros((1, 2, 64, 64), np.float32)
    ready, flags, h = C.c_int(), C.c_int(), C.c_void_p(1)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    with pytest.raises(_lib.B2FError, match="b2f_stream_open_ex: null context"):
        _lib.check(L.b2f_stream_open_ex(None, 1, back2future.IN_U8, 64, 64, back2future.STREAM_WARP, C.byref(h)))
    assert h.value is None
    with pytest.raises(_lib.B2FError, match="null out"):
        _lib.check(L.b2f_stream_open_ex(None, 1, back2future.IN_U8, 64, 64, 0, None))
    calls = [
        lambda: L.b2f_stream_push_warp(None, vp(u), 20.0, 0, vp(w), photo.ctypes.data_as(C.POINTER(C.c_ulonglong)), None, None, None, None, None,
                                       C.byref(ready)),
        lambda: L.b2f_stream_push_warp_device(None, vp(u), 20.0, 0, vp(w), vp(photo), None, None, None, None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_push_past(None, vp(u), _lib.fptr(flow), _lib.fptr(flow), None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_push_past_device(None, vp(u), vp(flow), vp(flow), None, None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_flags(None, C.byref(flags)),
    ]
    for call in calls:
        with pytest.raises(_lib.B2FError, match="null stream"):
            _lib.check(call())


class _NoLib(back2future.Model):
    def __init__(self):
        self._h = None
        self._streams = []


def _stream_without_library(cams=1, dtype=np.uint8, handle=1):
    st = object.__new__(back2future.MotionStream)
    st._h, st._model = handle, _NoLib()
    st.cams, st.H0, st.W0, st.dtype = cams, 64, 128, np.dtype(dtype)
    st.in_kind = back2future.IN_U8 if dtype == np.uint8 else back2future.IN_UNIT
    st.flags = back2future.STREAM_WARP | back2future.STREAM_PAST
    return st


def test_wrappers_validate_like_their_sequence_counterparts(monkeypatch):
    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_call)
    st = _stream_without_library()
    frame = np.zeros((3, 64, 128), np.uint8)
    for push in (st.pushWarp, st.pushPast):
        with pytest.raises(ValueError, match="expected 1 x 3 x 64 x 128"):
            push(np.zeros((3, 64, 64), np.uint8))
        with pytest.raises(ValueError, match="expected 1 x 3 x 64 x 128"):
            push(np.zeros((2, 3, 64, 128), np.uint8))
        with pytest.raises(ValueError, match="uint8 frames"):
            push(frame.astype(np.float32))
    # the messages of computeFlowSequenceWarp's checks, under the push's name
    with pytest.raises(ValueError, match="pushWarp: at least one of want_warped and want_photo"):
        st.pushWarp(frame, want_warped=False, want_photo=False)
    with pytest.raises(ValueError, match="pushWarp: want_past needs own_past_flow=True"):
        st.pushWarp(frame, want_past=True)
    with pytest.raises(ValueError, match="pushWarp: out must hold the 2 arrays"):
        st.pushWarp(frame, out=(np.zeros((1, 2, 3, 64, 128), np.uint8),))
    with pytest.raises(ValueError, match=r"pushWarp: out\[0\] must be a writeable C-contiguous uint8 array of shape \(1, 2, 3, 64, 128\)"):
        st.pushWarp(frame, out=(np.zeros((1, 2, 3, 64, 128), np.float32), np.zeros((1, 14), np.uint64)))
    with pytest.raises(ValueError, match=r"pushWarp: out\[1\] must be a writeable C-contiguous uint64 array of shape \(1, 14\)"):
        st.pushWarp(frame, out=(np.zeros((1, 2, 3, 64, 128), np.uint8), np.zeros((1, 13), np.uint64)))
    with pytest.raises(ValueError, match=r"pushWarp: out\[2\]"):   # the past flow is the last of (warped, photo, past_flow)
        st.pushWarp(frame, own_past_flow=True, want_past=True,
                    out=(np.zeros((1, 2, 3, 64, 128), np.uint8), np.zeros((1, 14), np.uint64), np.zeros((1, 2, 64, 64), np.float32)))
    # ... and of computeFlowSequencePast's
    with pytest.raises(ValueError, match=r"pushPast: out must be \(flow, past_flow, fwd_occ, bwd_occ\)"):
        st.pushPast(frame, out=(np.zeros((1, 2, 64, 128), np.float32),))
    with pytest.raises(ValueError, match=r"pushPast: out\[1\]"):
        st.pushPast(frame, out=(np.zeros((1, 2, 64, 128), np.float32), np.zeros((1, 2, 64, 128), np.float64), None, None))
    with pytest.raises(ValueError, match="required"):
        st.pushDeviceWarp(1 << 20)
    with pytest.raises(ValueError, match="required"):
        st.pushDevicePast(1 << 20, 1 << 20, 0)
    fl = _stream_without_library(cams=2, dtype=np.float32)
    with pytest.raises(ValueError, match=r"pushWarp: out\[0\] must be a writeable C-contiguous float32 array of shape \(2, 2, 3, 64, 128\)"):
        fl.pushWarp(np.zeros((2, 3, 64, 128), np.float32), want_photo=False, out=np.zeros((2, 2, 3, 64, 128), np.uint8))
    closed = _stream_without_library(handle=None)
    for call in (lambda: closed.pushWarp(frame), lambda: closed.pushPast(frame), lambda: closed.pushDeviceWarp(1 << 20, d_photo=1 << 20),
                 lambda: closed.pushDevicePast(1 << 20, 1 << 20, 1 << 20)):
        with pytest.raises(ValueError, match="closed"):
            call()
    for s in (st, fl):
        s._h = None   # nothing to free


# ---- the clips can tell the ring slots apart: a condition on the inputs of tests/test_gpu_stream_warp.py, not a measurement ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("H0,W0", SC.SIZES)
def test_the_frames_of_every_triplet_differ_pairwise(H0, W0, dtype):
    for seed in SC.SEEDS:
        V = SC.clip(seed, H0, W0, dtype)
        assert V.shape == (SC.T, 3, H0, W0) and V.dtype == dtype
        for k in range(2, SC.T):
            for a, b in ((k - 2, k - 1), (k - 1, k), (k - 2, k)):
                share = SC.differing_pixels(V[a], V[b])
                assert share > 0.5, "seed %d: frames %d and %d differ in %.3f of their pixels" % (seed, a, b, share)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("H0,W0", SC.SIZES)
def test_exchanging_two_frames_shows_in_the_host_definition(H0, W0, dtype):
    """past <-> future and past <-> reference, for every triplet: at least one photo word and more than 1 % of the warped samples
    change, so a push that reads a wrong slot cannot reproduce the sequence or the host definition"""
    flow, prob = SC.probe_flow(5, H0, W0)
    for seed in SC.SEEDS:
        V = SC.clip(seed, H0, W0, dtype)
        for k in range(2, SC.T):
            for swap, what in (((0, 2), "past <-> future"), ((0, 1), "past <-> reference")):
                share, words = SC.exchange_changes(V, k, flow, prob, swap)
                assert words >= 1 and share > 0.01, "seed %d, triplet %d, %s: %d words, %.4f of the samples" % (seed, k, what, words, share)
