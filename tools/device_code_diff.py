"""Are the GPU kernels of two source trees the same bytes?  The check of a host-only refactor.

    python tools/device_code_diff.py <parent tree> <this tree> [-j N] [--keep DIR]

Compiles every .hip of build.SOURCES (product flags) and of build.EXP_SOURCES (-DB2F_EXPERIMENTS=1) of both trees for the
device only, with the flags and the per-file EXTRA of <this tree>'s back2future_amd/build.py, copies .text, .rodata and .note
out of each device ELF and compares their hashes.  Prints `same` or `DIFFERENT` per file; exit status 1 on any difference.
A file that only one tree has is compiled there and printed as `new` (this tree's) or `gone` (the parent's); it is no difference.

The sections are compared, not the files, and both trees' builds of a file get the same -cuid.  By default hipcc hashes the paths
(the output's included) into a symbol __hip_cuid_<hex>, printed without leading zeros: besides making the whole ELFs differ, a
hash that comes out one digit shorter shortens .dynstr, which can move .rodata and .text across an alignment boundary, and the
kernel descriptors in .rodata hold the offset to their code.  Identical source then compared DIFFERENT in .rodata now and then.
With the id fixed per (build, file) the layout depends on the source and the flags alone.
Bytes are hashed; no instruction is looked at.  Needs hipcc and llvm-objcopy (ROCm), no GPU.
"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

SECTIONS = [".text", ".rodata", ".note"]


def load_build(tree):
    spec = importlib.util.spec_from_file_location("b2f_build_of_tree", os.path.join(tree, "back2future_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def find_objcopy(hipcc):
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-objcopy"), os.path.join(rocm, "llvm", "bin", "llvm-objcopy")):
        if os.path.exists(c):
            return c
    return shutil.which("llvm-objcopy") or sys.exit("llvm-objcopy not found")


def section_hashes(b, objcopy, tree, rel_dir, src, experiments, out_dir):
    """{section: sha256} of the device code of one source file of one tree"""
    # the same id in both trees, another per file and per build (hipcc hashes it once more into the symbol's name)
    cuid = hashlib.sha256(("%d/%s/%s" % (experiments, rel_dir, src)).encode()).hexdigest()[:16]
    csrc = os.path.join(tree, "back2future_amd", "csrc")
    elf = os.path.join(out_dir, src + ".elf")
    cmd = ([b.HIPCC] + b.FLAGS + (["-DB2F_EXPERIMENTS=1", "-I", csrc] if experiments else []) + b.EXTRA.get(src, []) +
           ["-cuid=" + cuid, "--offload-device-only", "--no-gpu-bundle-output", "-x", "hip", "-c", os.path.join(tree, rel_dir, src), "-o", elf])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (os.path.join(tree, rel_dir, src), r.stdout.decode()))
    h = {}
    for sec in SECTIONS:
        raw = elf + sec
        subprocess.check_call([objcopy, "-O", "binary", "--only-section=" + sec, elf, raw])
        with open(raw, "rb") as f:
            h[sec] = hashlib.sha256(f.read()).hexdigest()
    return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1), help="compilations at a time")
    ap.add_argument("--keep", help="keep the device ELFs and section files in this directory")
    a = ap.parse_args()
    trees = [os.path.abspath(a.parent), os.path.abspath(a.this)]
    b, b_parent = load_build(trees[1]), load_build(trees[0])
    objcopy = find_objcopy(b.HIPCC)
    csrc_rel = os.path.join("back2future_amd", "csrc")
    exp_rel = os.path.relpath(b.EXP_DIR, trees[1])
    # (label, directory in the tree, file, experiments build)
    units = [("product", csrc_rel, s, False) for s in b.SOURCES if s.endswith(".hip")]
    units += [("experiments", csrc_rel, s, True) for s in b.SOURCES if s.endswith(".hip")]
    units += [("experiments", exp_rel, s, True) for s in b.EXP_SOURCES if s.endswith(".hip")]
    # files only the parent lists (`gone`), after this tree's
    units += [("product", csrc_rel, s, False) for s in b_parent.SOURCES if s.endswith(".hip") and s not in b.SOURCES]
    units += [("experiments", csrc_rel, s, True) for s in b_parent.SOURCES if s.endswith(".hip") and s not in b.SOURCES]
    units += [("experiments", exp_rel, s, True) for s in b_parent.EXP_SOURCES if s.endswith(".hip") and s not in b.EXP_SOURCES]
    work = a.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    different = 0
    try:
        with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
            jobs = []
            for label, rel, src, exp in units:
                fut = []
                for i, tree in enumerate(trees):
                    d = os.path.join(work, "parent" if i == 0 else "this", label)
                    os.makedirs(d, exist_ok=True)
                    there = os.path.exists(os.path.join(tree, rel, src))
                    fut.append(pool.submit(section_hashes, b, objcopy, tree, rel, src, exp, d) if there else None)
                jobs.append((label, src, fut))
            for label, src, (fa, fb) in jobs:
                if fa is None or fb is None:
                    (fa or fb).result()
                    print("%-12s %-28s %s" % (label, src, "new" if fa is None else "gone"), flush=True)
                    continue
                ha, hb = fa.result(), fb.result()
                diff = [s for s in SECTIONS if ha[s] != hb[s]]
                different += bool(diff)
                print("%-12s %-28s %s" % (label, src, "DIFFERENT in " + " ".join(diff) if diff else "same"), flush=True)
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)
    print("%d of %d device builds differ" % (different, len(units)))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
