"""CPU: the stream entry points (b2f_stream_*) are declared, exported, bound and usable from C; FlowStream refuses malformed input
before any library call; every entry fails loudly on a NULL stream or context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["b2f_stream_open", "b2f_stream_reset", "b2f_stream_info", "b2f_stream_push", "b2f_stream_push_rgb", "b2f_stream_push_device"]
NAMES = INT_NAMES + ["b2f_stream_close"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def test_header_declares_the_stream_entry_points():
    src = open(os.path.join(ROOT, "include", "b2f.h")).read()
    for n in INT_NAMES:
        assert re.search(r"B2F_API\s+int\s+%s\s*\(" % n, src), n
    assert re.search(r"B2F_API\s+void\s+b2f_stream_close\s*\(\s*b2f_stream\s*\*", src)
    assert re.search(r"typedef\s+struct\s+b2f_stream\s+b2f_stream\s*;", src)
    assert "back2future.lua:47-95" in src[src.index("typedef struct b2f_stream"):]   # names the calling pattern it replaces


def test_library_exports_and_binds_them():
    L = C.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n


C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "b2f.h"
int main(void)
{
    static unsigned char u[3 * 64 * 64], rgb[3 * 64 * 64];
    static float flow[2 * 64 * 64];
    b2f_stream *st = (b2f_stream *)u;
    int ready = 5, cams = 0;
    long long pushed = 0;
    int rc = b2f_stream_open(NULL, 1, B2F_IN_U8, 64, 64, &st);
    if (st != NULL || strstr(b2f_last_error(), "null context") == NULL) return 2;
    rc += b2f_stream_push(NULL, u, flow, NULL, NULL, NULL, &ready);
    if (strstr(b2f_last_error(), "null stream") == NULL) return 3;
    rc += b2f_stream_push_rgb(NULL, u, 0.0, B2F_RGB_PACKED, rgb, NULL, NULL, NULL, NULL, &ready);
    rc += b2f_stream_push_device(NULL, u, flow, NULL, NULL, NULL, NULL, &ready);
    rc += b2f_stream_reset(NULL);
    rc += b2f_stream_info(NULL, &cams, NULL, NULL, NULL, &pushed);
    b2f_stream_close(NULL);
    printf("%d %s\n", rc, b2f_last_error());
    return rc == 6 ? 0 : 1;
}
"""


def test_c99_program_calls_them(tmp_path):
    src = tmp_path / "stream.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "stream")
    lib_dir = os.path.join(ROOT, "back2future_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", exe, "-L" + lib_dir, "-lb2f", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "null stream" in r.stdout


def test_entry_points_fail_loudly_on_a_null_stream_or_context():
    L = _lib.lib()
    u = np.zeros((1, 3, 64, 64), np.uint8)
    flow = np.zeros((1, 2, 64, 64), np.float32)
    rgb = np.zeros((1, 3, 64, 64), np.uint8)
    ready, h = C.c_int(), C.c_void_p(1)
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    with pytest.raises(_lib.B2FError, match="null context"):
        _lib.check(L.b2f_stream_open(None, 1, back2future.IN_U8, 64, 64, C.byref(h)))
    assert h.value is None
    with pytest.raises(_lib.B2FError, match="null out"):
        _lib.check(L.b2f_stream_open(None, 1, back2future.IN_U8, 64, 64, None))
    calls = [
        lambda: L.b2f_stream_push(None, vp(u), _lib.fptr(flow), None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_push_rgb(None, vp(u), 0.0, 0, up(rgb), None, None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_push_device(None, vp(u), vp(flow), None, None, None, None, C.byref(ready)),
        lambda: L.b2f_stream_reset(None),
        lambda: L.b2f_stream_info(None, None, None, None, None, None),
    ]
    for call in calls:
        with pytest.raises(_lib.B2FError, match="null stream"):
            _lib.check(call())
    L.b2f_stream_close(None)   # a no-op


class _NoLib(back2future.Model):
    """A Model without a context: any library call would fail, so these checks run before one."""

    def __init__(self):
        self._h = None
        self._streams = []


def _stream_without_library(cams=1, dtype=np.uint8, handle=1):
    st = object.__new__(back2future.FlowStream)
    st._h, st._model = handle, _NoLib()
    st.cams, st.H0, st.W0, st.dtype = cams, 64, 128, np.dtype(dtype)
    st.in_kind = back2future.IN_U8 if dtype == np.uint8 else back2future.IN_UNIT
    return st


def test_wrappers_reject_bad_input_before_calling_the_library(monkeypatch):
    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_call)
    m = _NoLib()
    with pytest.raises(ValueError, match="closed"):
        m.openStream(64, 128)
    m._h = 1
    for kw, match in [(dict(dtype=np.float64), "dtype"), (dict(dtype="nonsense"), "dtype"), (dict(cams=0), "cams"), (dict(H0=32), "H0")]:
        args = dict(H0=64, W0=128)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            m.openStream(**args)
    m._h = None
    st = _stream_without_library()
    frame = np.zeros((3, 64, 128), np.uint8)
    for push in (st.push, st.pushRGB):
        with pytest.raises(ValueError, match="expected 1 x 3 x 64 x 128"):
            push(np.zeros((3, 64, 64), np.uint8))
        with pytest.raises(ValueError, match="expected 1 x 3 x 64 x 128"):
            push(np.zeros((2, 3, 64, 128), np.uint8))
        with pytest.raises(ValueError, match="uint8 frames"):
            push(frame.astype(np.float32))
    with pytest.raises(ValueError, match="out must be"):
        st.push(frame, out=(np.zeros((1, 2, 64, 128), np.float32),))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        st.push(frame, out=(np.zeros((1, 2, 64, 128), np.float64), None, None))
    with pytest.raises(ValueError, match="max must be"):
        st.pushRGB(frame, max=-1)
    with pytest.raises(ValueError, match="required"):
        st.pushDevice(0, 1 << 20)
    two = _stream_without_library(cams=2, dtype=np.float32)
    with pytest.raises(ValueError, match="expected 2 x 3 x 64 x 128"):
        two.push(np.zeros((3, 64, 128), np.float32))     # one frame for two cameras
    with pytest.raises(ValueError, match="float32 frames"):
        two.push(np.zeros((2, 3, 64, 128), np.uint8))
    closed = _stream_without_library(handle=None)
    for call in (lambda: closed.push(frame), lambda: closed.pushRGB(frame), lambda: closed.pushDevice(1 << 20, 1 << 20), closed.reset,
                 lambda: closed.frames_pushed):
        with pytest.raises(ValueError, match="closed"):
            call()
    closed.close()   # closing twice is fine
    for s in (st, two):
        s._h = None  # nothing to free
