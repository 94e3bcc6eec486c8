"""The reference's own bilinear sampler, compiled for the GPU: extras/stnbhwd/BilinearSamplerBHWD.cu, unmodified, behind
oracle/ref/ref_sampler.cpp and the two shim headers of oracle/ref/shim/ (stand-ins for <lua.h> and "THCGeneral.h").

TEST INFRASTRUCTURE ONLY.  build() compiles two libraries into oracle/_ref/ (git-ignored; nothing of the reference is committed):
  libref_sampler.so       -ffp-contract=off, the flags of libb2f.so and of the CPU oracle: the authority on the ORDER of operations
  libref_sampler_fma.so   hipcc's default contraction: what a default build of the reference may do to the same expressions
The reference checkout is $B2F_REFERENCE_DIR (default /root/reference).  Where it is absent build() uses what oracle/_ref/ already
holds and returns None if that is nothing.  The wrappers need a GPU; layouts are the module's (BHWD images, BHW(xy) grids)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "ref")
OUT = os.path.join(_HERE, "_ref")
DRIVER = os.path.join(SRC, "ref_sampler.cpp")
SHIM = os.path.join(SRC, "shim")
SAMPLER_DIR = os.path.join("extras", "stnbhwd")
SAMPLER = "BilinearSamplerBHWD.cu"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-unused-result"]
# library -> what it adds to FLAGS
VARIANTS = {"libref_sampler.so": ["-ffp-contract=off"], "libref_sampler_fma.so": []}
ENTRIES = ("ref_sampler_forward", "ref_sampler_backward", "ref_sampler_backward_only_grid")
_libs = {}


def reference_dir():
    return os.environ.get("B2F_REFERENCE_DIR", "/root/reference")


def lib_path(fma=False):
    return os.path.join(OUT, "libref_sampler_fma.so" if fma else "libref_sampler.so")


def _sources():
    return [DRIVER] + sorted(os.path.join(SHIM, f) for f in os.listdir(SHIM))


def build(force=False, verbose=False):
    """-> the path of libref_sampler.so (both libraries exist then), or None where there is neither a reference checkout nor an earlier build"""
    src_dir = os.path.join(reference_dir(), SAMPLER_DIR)
    have = all(os.path.exists(os.path.join(OUT, name)) for name in VARIANTS)
    if not os.path.exists(os.path.join(src_dir, SAMPLER)):
        return lib_path() if have else None
    os.makedirs(OUT, exist_ok=True)
    deps = _sources() + [os.path.join(src_dir, SAMPLER), os.path.join(src_dir, "utils.h")]
    newest = max(os.path.getmtime(d) for d in deps)
    procs = []
    for name, extra in VARIANTS.items():
        target = os.path.join(OUT, name)
        if not force and os.path.exists(target) and os.path.getmtime(target) >= newest:
            continue
        obj = os.path.splitext(target)[0] + ".o"
        cmd = [HIPCC] + FLAGS + extra + ["-I", SHIM, "-I", src_dir, "-x", "hip", "-c", DRIVER, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((target, obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for target, obj, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed on %s:\n%s\n" % (os.path.basename(target), out.decode()))
        elif verbose and out.strip():
            print(out.decode())
    if failed:
        raise RuntimeError("reference sampler build failed")
    for target, obj, _ in procs:
        # linked as back2future_amd/build.py links libb2f.so
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target, obj, "-ldl", "-lpthread"])
    return lib_path()


def lib(fma=False):
    key = bool(fma)
    if key not in _libs:
        if not os.path.exists(lib_path(fma)):          # loading never builds: build() is __graft_entry__.build()'s step
            raise RuntimeError("%s does not exist: run oracle.reference.build() with a reference checkout" % lib_path(fma))
        _libs[key] = C.CDLL(lib_path(fma))
    return _libs[key]


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %d (> 0: the HIP error; -1: bad arguments; -2: the reference called THError)" % (what, rc))


def forward(img, grid, fma=False):
    """BilinearSamplerBHWD:updateOutput: img B x ih x iw x C, grid B x gh x gw x 2 (x first) -> B x gh x gw x C"""
    img, ip = _f(img); grid, gp = _f(grid)
    B, ih, iw, c = img.shape
    _, gh, gw, two = grid.shape
    assert two == 2 and grid.shape[0] == B
    out = np.empty((B, gh, gw, c), np.float32)
    _check(lib(fma).ref_sampler_forward(ip, gp, B, ih, iw, c, gh, gw, out.ctypes.data_as(C.POINTER(C.c_float))), "ref_sampler_forward")
    return out


def backward(img, grid, grad_out, only_grid=False, fma=False):
    """BilinearSamplerBHWD:updateGradInput (only_grid: its OnlyGrid form); returns (grad_img or None, grad_grid)"""
    img, ip = _f(img); grid, gp = _f(grid); grad_out, op = _f(grad_out)
    B, ih, iw, c = img.shape
    _, gh, gw, two = grid.shape
    assert two == 2 and grid.shape[0] == B and grad_out.shape == (B, gh, gw, c)
    gg = np.empty_like(grid)
    ggp = gg.ctypes.data_as(C.POINTER(C.c_float))
    if only_grid:
        _check(lib(fma).ref_sampler_backward_only_grid(ip, gp, op, B, ih, iw, c, gh, gw, ggp), "ref_sampler_backward_only_grid")
        return None, gg
    gi = np.empty_like(img)
    _check(lib(fma).ref_sampler_backward(ip, gp, op, B, ih, iw, c, gh, gw, gi.ctypes.data_as(C.POINTER(C.c_float)), ggp), "ref_sampler_backward")
    return gi, gg


def warping_unit(I, F, k, fma=False):
    """warpingUnit(I, MulConstant(k)(F)) of models/pwc.lua:67-73: I B x C x h x w, F B x 2 x h x w -> B x C x h x w.  The transposes and the
    float32 product by k are numpy's; the sampler between them is the compiled reference."""
    I = np.asarray(I, np.float32)
    F = (np.asarray(F, np.float32) * np.float32(k)).astype(np.float32)
    out = forward(np.transpose(I, (0, 2, 3, 1)), np.transpose(F, (0, 2, 3, 1)), fma)
    return np.ascontiguousarray(np.transpose(out, (0, 3, 1, 2)))


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
