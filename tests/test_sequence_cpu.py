"""CPU: the sequence entry points (b2f_forward_sequence_device, b2f_compute_flow_sequence[_u8] and their b2f_multi forms) are
declared, exported, bound and usable from C; the Python wrappers refuse malformed input before any library call; the entry
points fail loudly on a NULL context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["b2f_forward_sequence_device", "b2f_compute_flow_sequence", "b2f_compute_flow_sequence_u8",
         "b2f_multi_compute_flow_sequence", "b2f_multi_compute_flow_sequence_u8"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def test_header_declares_the_sequence_entry_points():
    src = open(os.path.join(ROOT, "include", "b2f.h")).read()
    for n in NAMES:
        assert re.search(r"B2F_API\s+int\s+%s\s*\(" % n, src), n
    assert re.search(r"enum\s*\{\s*B2F_IN_U8\s*=\s*2\s*\}", src)
    assert back2future.IN_U8 == 2 and back2future.IN_UNIT == 1 and back2future.IN_NORMALIZED == 0


def test_library_exports_and_binds_them():
    L = C.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n


C_PROGRAM = r"""
#include <stdio.h>
#include "b2f.h"
int main(void)
{
    static float f[3 * 3 * 64 * 64];
    static unsigned char u[3 * 3 * 64 * 64];
    static double flow[2 * 64 * 64];
    static unsigned char fo[64 * 64], bo[64 * 64];
    int rc = b2f_compute_flow_sequence(NULL, 3, f, 64, 64, flow, fo, bo);
    rc += b2f_compute_flow_sequence_u8(NULL, 3, u, 64, 64, flow, fo, bo);
    rc += b2f_multi_compute_flow_sequence(NULL, 3, f, 64, 64, flow, fo, bo);
    rc += b2f_multi_compute_flow_sequence_u8(NULL, 3, u, 64, 64, flow, fo, bo);
    rc += b2f_forward_sequence_device(NULL, f, B2F_IN_U8, 3, 64, 64, NULL, NULL, NULL, NULL);
    printf("%d %s\n", rc, b2f_last_error());
    return rc == 5 ? 0 : 1;
}
"""


def test_c99_program_calls_them(tmp_path):
    src = tmp_path / "seq.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "seq")
    lib_dir = os.path.join(ROOT, "back2future_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", exe, "-L" + lib_dir, "-lb2f", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "null" in r.stdout


class _NoLib(back2future.Model):
    """A Model without a context: any library call would fail, so these checks run before one."""

    def __init__(self):
        self._h = None


class _NoLibMulti(back2future.MultiModel):
    def __init__(self):
        self._h = None


@pytest.mark.parametrize("cls", [_NoLib, _NoLibMulti])
def test_wrappers_reject_bad_sequences_before_calling_the_library(cls, monkeypatch):
    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_call)
    m = cls()
    with pytest.raises(ValueError, match="T >= 3"):
        m.computeFlowSequence(np.zeros((2, 3, 64, 64), np.float32))
    with pytest.raises(ValueError, match="T >= 3"):
        m.computeFlowSequence([np.zeros((3, 64, 64), np.uint8)] * 2)
    with pytest.raises(ValueError, match="3 x H x W"):
        m.computeFlowSequence(np.zeros((4, 1, 64, 64), np.float32))
    with pytest.raises(ValueError, match="3 x H x W"):
        m.computeFlowSequence([np.zeros((4, 64, 64), np.float32)] * 4)
    with pytest.raises(ValueError, match="mixed dtypes"):
        m.computeFlowSequence([np.zeros((3, 64, 64), np.float32), np.zeros((3, 64, 64), np.uint8),
                               np.zeros((3, 64, 64), np.float32)])
    with pytest.raises(ValueError, match="same size"):
        m.computeFlowSequence([np.zeros((3, 64, 64), np.float32)] * 2 + [np.zeros((3, 64, 128), np.float32)])
    if cls is _NoLib:
        with pytest.raises(ValueError, match="T >= 3"):
            m.forward_sequence_device(1 << 20, 2, 64, 64)


def test_sequence_frames_keeps_the_dtype():
    v, b = back2future.sequence_frames([np.zeros((3, 4, 5), np.uint8)] * 3)
    assert b and v.dtype == np.uint8 and v.shape == (3, 3, 4, 5) and v.flags.c_contiguous
    v, b = back2future.sequence_frames(np.zeros((4, 3, 4, 5), np.float64))
    assert not b and v.dtype == np.float32 and v.shape == (4, 3, 4, 5)


def test_entry_points_fail_loudly_on_a_null_context():
    L = _lib.lib()
    f = np.zeros((3, 3, 64, 64), np.float32)
    u = np.zeros((3, 3, 64, 64), np.uint8)
    flow = np.zeros((1, 2, 64, 64), np.float64)
    fo, bo = np.zeros((1, 64, 64), np.uint8), np.zeros((1, 64, 64), np.uint8)
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    dp = flow.ctypes.data_as(C.POINTER(C.c_double))
    calls = [
        lambda: L.b2f_compute_flow_sequence(None, 3, _lib.fptr(f), 64, 64, dp, up(fo), up(bo)),
        lambda: L.b2f_compute_flow_sequence_u8(None, 3, up(u), 64, 64, dp, up(fo), up(bo)),
        lambda: L.b2f_multi_compute_flow_sequence(None, 3, _lib.fptr(f), 64, 64, dp, up(fo), up(bo)),
        lambda: L.b2f_multi_compute_flow_sequence_u8(None, 3, up(u), 64, 64, dp, up(fo), up(bo)),
        lambda: L.b2f_forward_sequence_device(None, C.c_void_p(f.ctypes.data), 1, 3, 64, 64, None, None, None, None),
    ]
    for call in calls:
        with pytest.raises(_lib.B2FError, match="null"):
            _lib.check(call())
