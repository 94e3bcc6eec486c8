"""Deterministic text report of what the library's host-side dispatch decides (GPU box only): which kernel runs every conv of a
forward pass (the profile rows: name, launch count) and the bits it produces (sha256), over shapes, batch sizes and the kernel
options; the op entry b2f_op_conv3x3 on the shape lists of the parity tests; and every option as b2f_get_option reports it after
init from the environment and after b2f_set_option.  Two builds that decide and compute the same give the same report:

    python tools/dispatch_snapshot.py > a.txt
    B2F_LIB=/other/build/libb2f.so python tools/dispatch_snapshot.py > b.txt && diff a.txt b.txt

Not a test: it asserts nothing.  Sections that need their own environment run as child processes (--child NAME), one at a time,
each under a time limit; the report stops at the first one that fails.
"""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if sys.argv[1:] != ["--child", "dump"]:
    import torch  # noqa: F401  before libb2f.so loads: torch finds the GPU only through its own libamdhip64
import numpy as np
from back2future_amd import back2future, ops
from back2future_amd._lib import B2FError

HARD, SOFT = "random:hard:2:1.0", "random:soft:2:1.0"
# every b2f_set_option key, and the ones b2f_init seeds from B2F_<NAME>
KEYS = ["use_graph", "host_graph", "profile", "profile_layers", "bf16_direct", "bf16_conv", "bf16_conv_min_pixels", "wino1d", "wino6",
        "wino6_min_pixels", "wino2_split", "wino4_split", "wino4_hybrid", "s2_tiles_per_block", "wino4_persistent", "s2_loader",
        "s2_tile_groups", "wino_split_pixels", "wino8", "wino4_min_pixels", "adaptive_kernels", "corr_variant", "corr_ablate",
        "op_wino_split", "op_gradw_partials", "op_hole_fill", "host_subbatch_pixels", "host_threads", "host_u8", "host_ramp", "debug_fail_next"]
UNSEEDED = ["bf16_conv_min_pixels", "op_hole_fill", "debug_fail_next"]
EXPERIMENT_ONLY = ["wino2_split", "wino4_split", "wino4_hybrid"]
OPTION_MATRIX = [
    {"wino6": 0}, {"wino6": 0, "wino4_min_pixels": 0}, {"wino4_min_pixels": 1000000}, {"adaptive_kernels": 0}, {"adaptive_kernels": 1},
    {"wino1d": 1}, {"wino1d": 2}, {"bf16_conv": 0, "bf16_conv_min_pixels": 1024}, {"bf16_conv": 2, "bf16_conv_min_pixels": 1024},
    {"bf16_conv": 3, "bf16_conv_min_pixels": 1024}, {"bf16_direct": 0}, {"s2_loader": 0}, {"s2_loader": 2}, {"s2_tile_groups": 0},
    {"wino8": 0}, {"wino_split_pixels": 0}, {"wino4_persistent": 0}, {"wino4_persistent": 3}, {"s2_tiles_per_block": 2},
    {"wino6_min_pixels": 4096}]
# (ci, co, stride, h, w, batch) of tests/test_gpu_parity.py: test_conv3x3, test_conv3x3_wino6, test_stride2_loader_consumer_kernel,
# test_direct_conv_on_the_bf16_pipe
OP_SHAPES = {
    "conv3x3": [(ci, co, s, h, w, 2) for (ci, co, s, h, w) in [
        (3, 16, 2, 64, 96), (16, 16, 1, 32, 48), (32, 64, 2, 24, 40), (96, 96, 1, 9, 30), (128, 192, 2, 8, 14), (192, 192, 1, 4, 7),
        (196, 128, 1, 16, 33), (32, 2, 1, 20, 17), (5, 7, 1, 3, 5), (64, 32, 1, 1, 2), (64, 64, 1, 40, 70), (8, 68, 1, 18, 34),
        (128, 128, 1, 33, 65), (16, 16, 1, 5, 37), (16, 16, 1, 35, 66), (32, 2, 1, 33, 18), (40, 32, 1, 17, 33), (24, 96, 1, 20, 40),
        (16, 32, 2, 24, 40), (16, 32, 2, 9, 33), (16, 32, 2, 7, 131), (16, 32, 2, 1, 1), (16, 32, 2, 18, 64), (12, 32, 2, 10, 12)]],
    "wino6": [(ci, co, 1, h, w, 3) for (ci, co, h, w) in [
        (128, 128, 40, 70), (200, 128, 33, 65), (32, 64, 17, 100), (104, 192, 48, 33), (64, 100, 70, 31), (40, 160, 16, 32), (32, 32, 49, 35),
        (128, 96, 36, 83), (64, 32, 20, 70), (232, 128, 12, 48), (264, 128, 6, 6), (72, 36, 25, 49)]],
    "s2_loader": [(ci, co, 2, h, w, B) for (B, ci, co, h, w) in [
        (1, 64, 96, 16, 64), (2, 32, 64, 37, 71), (1, 64, 96, 33, 50), (3, 96, 128, 9, 130), (1, 128, 192, 32, 60), (2, 40, 64, 20, 20),
        (1, 64, 100, 31, 33), (1, 24, 32, 40, 66), (1, 8, 256, 2, 2), (4, 16, 36, 1, 1), (3, 72, 160, 64, 48), (1, 64, 96, 8, 16)]],
    "bf16_pipe": [(ci, co, s, h, w, B) for (B, ci, co, h, w, s) in [
        (1, 32, 64, 16, 64, 2), (2, 32, 64, 37, 71, 2), (1, 64, 96, 33, 50, 2), (3, 96, 128, 9, 130, 2), (1, 128, 192, 32, 60, 2),
        (2, 40, 64, 20, 20, 2), (1, 64, 100, 31, 33, 2), (1, 24, 32, 40, 66, 2), (1, 64, 32, 40, 66, 1)]],
}
OP_OPTIONS = [{}, {"wino6": 0}, {"wino1d": 1}, {"bf16_conv": 0}, {"s2_loader": 0}]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def opts_str(kv):
    return ",".join("%s=%d" % (k, v) for k, v in kv.items()) or "defaults"


def profiled(m):
    m.set_option("use_graph", 0)
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    return m


def print_rows(m):
    for name, (_, n) in sorted(m.profile_read().items()):
        if n:
            print("    %-32s x%d" % (name, n))


def forward(m, B, H, W, seq=False):
    """One forward_device (or, with seq, forward_sequence_device on B + 2 frames) on deterministic inputs: profile rows and output hashes."""
    dev = torch.device("cuda", 0)
    r = np.random.default_rng(B * 1000003 + H * 1009 + W + (7 if seq else 0))
    x = torch.from_numpy(r.random((B + 2, 3, H, W) if seq else (B, 9, H, W), dtype=np.float32)).to(dev)
    flow = torch.zeros(B, 2, H, W, device=dev)
    occ = torch.zeros(B, 2, H, W, device=dev)
    est3 = torch.zeros(B, 2 if m.past_flow else 3, H, W, device=dev)
    torch.cuda.synchronize()
    m.profile_reset()
    if seq:
        m.forward_sequence_device(x.data_ptr(), B + 2, H, W, flow.data_ptr(), occ.data_ptr(), est3.data_ptr(), in_kind=back2future.IN_UNIT)
    else:
        m.forward_device(x.data_ptr(), B, H, W, flow.data_ptr(), occ.data_ptr(), est3.data_ptr(), unit_input=True)
    m.synchronize()
    print("  %s B=%d %dx%d" % ("sequence" if seq else "forward", B, H, W))
    print_rows(m)
    print("    flow %s occ %s est3 %s" % (sha(flow.cpu().numpy()), sha(occ.cpu().numpy()), sha(est3.cpu().numpy())))


def full_table(m, B, H, W):
    r = np.random.default_rng(B * 31 + H + W)
    x = r.standard_normal((B, 9, H, W), dtype=np.float32)
    m.profile_reset()
    outs = m.forward(x)
    print("  full table B=%d %dx%d" % (B, H, W))
    print_rows(m)
    print("    outputs " + " ".join(sha(o) for o in outs))


def section_forwards():
    for name in (HARD, SOFT):
        m = profiled(back2future.Model(name))
        print("model %s" % name)
        for (B, H, W) in [(1, 128, 192), (2, 128, 192), (1, 512, 512), (2, 512, 512)]:
            forward(m, B, H, W)
        forward(m, 2, 128, 192, seq=True)     # T = 4
        full_table(m, 1, 128, 192)
        m.close()
    m = profiled(back2future.Model(HARD, graph="win=5,levels=4,skip=2"))
    print("model %s graph win=5,levels=4,skip=2" % HARD)
    full_table(m, 2, 64, 128)
    m.close()


def section_option_matrix():
    m = profiled(back2future.Model(HARD))
    for kv in OPTION_MATRIX:
        print("options %s" % opts_str(kv))
        with m.options(**kv):
            for (B, H, W) in [(2, 128, 192), (1, 512, 512), (2, 512, 512)]:
                forward(m, B, H, W)
    m.close()


def section_wino0():
    """child process with B2F_WINO=0"""
    m = profiled(back2future.Model(HARD))
    for (B, H, W) in [(2, 128, 192), (1, 512, 512)]:
        forward(m, B, H, W)
    m.close()


def section_ops():
    m = back2future.Model(HARD)
    for kv in OP_OPTIONS:
        print("op options %s" % opts_str(kv))
        with m.options(**kv):
            for lst, shapes in OP_SHAPES.items():
                for (ci, co, s, h, w, B) in shapes:
                    r = np.random.default_rng(ci * 1000 + co * 7 + h)
                    x = r.standard_normal((B, ci, h, w), dtype=np.float32)
                    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
                    b = r.standard_normal(co, dtype=np.float32)
                    print("  %-10s %3d->%-3d s%d %3dx%-3d B=%d  %s" % (lst, ci, co, s, h, w, B, sha(ops.conv3x3(m, x, wt, b, s, True))))
    m.close()


def dump(m):
    print("  " + " ".join("%s=%d" % (k, m.get_option(k)) for k in KEYS + ["experiments"]))


def section_dump():
    """child process: the options of a fresh context under this process's environment"""
    m = back2future.Model(HARD)
    dump(m)
    m.close()


def section_set_get():
    m = back2future.Model(HARD)
    exp = m.get_option("experiments")
    for k in KEYS:
        v = 0 if (k in EXPERIMENT_ONLY and not exp) else 3
        m.set_option(k, v)
        print("  set %s=%d -> %d" % (k, v, m.get_option(k)))
    m.set_option("host_subbatch_pixels", 0)
    print("  set host_subbatch_pixels=0 -> %d" % m.get_option("host_subbatch_pixels"))
    dump(m)
    for k, v in [("corr_variant", 2), ("corr_variant", 4), ("corr_variant", 6), ("corr_variant", 8), ("bf16_direct", 1), ("wino2_split", 1),
                 ("wino4_split", 1), ("wino4_hybrid", 1), ("experiments", 1), ("no_such_option", 1)]:
        try:
            m.set_option(k, v)
            print("  set %s=%d accepted -> %d" % (k, v, m.get_option(k)))
        except B2FError as e:
            print("  set %s=%d refused: %s" % (k, v, e))
    try:
        m.get_option("no_such_option")
    except B2FError as e:
        print("  get no_such_option refused: %s" % e)
    m.close()


CHILDREN = {"wino0": section_wino0, "dump": section_dump}


def child(name, env_extra, title):
    """Runs a section in a fresh process under a cleaned environment plus env_extra; b2f_init's warnings on stderr are part of the report."""
    print(title)
    sys.stdout.flush()
    env = {k: v for k, v in os.environ.items() if not k.startswith("B2F_") or k == "B2F_LIB"}
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    for line in p.stderr.decode().splitlines():   # the library's own messages belong to the report, the runtime's chatter does not
        print(line, file=sys.stdout if line.startswith("b2f_") else sys.stderr)
    sys.stdout.write(p.stdout.decode())
    if p.returncode != 0:
        print("child %s failed with exit status %d: report ends here" % (name, p.returncode))
        sys.exit(1)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        CHILDREN[sys.argv[2]]()
        return
    print("== model forwards")
    section_forwards()
    print("== option matrix (model %s)" % HARD)
    section_option_matrix()
    child("wino0", {"B2F_WINO": "0"}, "options B2F_WINO=0 (environment)")
    print("== op entry b2f_op_conv3x3")
    section_ops()
    print("== options")
    seeded = [k for k in KEYS if k not in UNSEEDED]
    child("dump", {}, "clean environment")
    for k in seeded:
        child("dump", {"B2F_" + k.upper(): "3"}, "B2F_%s=3" % k.upper())
    child("dump", {"B2F_" + k.upper(): "3" for k in seeded}, "every seeded option = 3")
    child("dump", {"B2F_CORR_LAT": "1"}, "B2F_CORR_LAT=1")
    child("dump", {"B2F_PROFILE_LAYERS": "yes"}, "B2F_PROFILE_LAYERS=yes")
    child("dump", {"B2F_CORR_VARIANT": "4", "B2F_BF16_DIRECT": "1"}, "B2F_CORR_VARIANT=4 B2F_BF16_DIRECT=1")
    print("set_option / get_option")
    section_set_get()


if __name__ == "__main__":
    main()
