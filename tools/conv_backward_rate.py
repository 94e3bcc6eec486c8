"""What the backward pass of a stride-1 conv layer costs on the GPU (GPU box only): ops.conv3x3_backward (csrc/b2f_convbwd.hip) on the
decoder layers 128 -> 128, 128 -> 96 and 200 -> 128 at 256 x 480 (level 3 of 1024 x 1920), batch 4, next to the forward layer on the
same data.

    python tools/conv_backward_rate.py [--n 4] [--height 256] [--width 480] [--reps 5] [--layout 1]

Prints ONE JSON line.  Every time is a profile row of the op entry (device events around the launches, option profile = 1), the median
over `reps` calls after one warm-up call; the host staging of the entry is not in it.  Per layer:
  gradinput             the gradInput conv: the forward kernel that ran (its row name) and its time
  mask, gradw, reduce   rows convbwd_mask, convbwd_gradw (conv3x3_gradw + gradb_partials), convbwd_reduce; partials, longest_chain: the plan
  forward_default       ops.conv3x3 with LeakyReLU under the default options: row name and time
  forward_direct        the same on the direct fp32 MFMA kernel (conv3x3_mfma): a child process with B2F_WINO=0 and bf16_conv = 0, the
                        only switch that sends a wide stride-1 layer there; the yardstick of gradw: same FLOP count, same instruction
  gradw_tflops, gradw_share_of_peak   2 * 9 * Ci * Co * B * H * W FLOP over gradw + reduce, and that over the fp32 matrix peak 157.3 TFLOP/s
  gradw_over_forward_direct           (gradw + reduce) / forward_direct
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from back2future_amd import back2future, ops

LAYERS = [(128, 128), (128, 96), (200, 128)]          # (Ci, Co)
FP32_MATRIX_PEAK = 157.3e12


def layer_data(ci, co, n, H, W):
    r = np.random.default_rng([7, ci, co, n, H, W])
    x = r.standard_normal((n, ci, H, W), dtype=np.float32)
    w = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    gy = r.standard_normal((n, co, H, W), dtype=np.float32)
    return x, w, b, gy


def row_medians(m, call, reps):
    """{row: median ms over reps calls} of the profile rows one call leaves, after a warm-up call; (result of the last call, rows)"""
    out = call()
    per = {}
    for _ in range(reps):
        m.profile_reset()
        out = call()
        for name, (ms, cnt) in m.profile_read().items():
            if cnt > 0:
                per.setdefault(name, []).append(ms)
    return out, {k: statistics.median(v) for k, v in per.items() if len(v) == reps}


def forward_row(m, x, w, b, reps):
    y, rows = row_medians(m, lambda: ops.conv3x3(m, x, w, b, 1, True), reps)
    conv = [k for k in rows if k.startswith("conv") and not k.startswith("convbwd_")]
    assert len(conv) == 1, rows
    return y, {"row": conv[0], "ms": round(rows[conv[0]], 4)}


def child_direct(a):
    m = back2future.Model("random:hard:2:1.0")
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    m.set_option("bf16_conv", 0)
    res = {}
    for ci, co in LAYERS:
        x, w, b, _ = layer_data(ci, co, a.n, a.height, a.width)
        _, row = forward_row(m, x, w, b, a.reps)
        if not row["row"].startswith("convD1_"):
            sys.exit("the forward layer ran %s, not the direct fp32 MFMA kernel" % row["row"])
        res["%dto%d" % (ci, co)] = row
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layout", type=int, default=1, help="1: the forward's chunk-planar strides, 0: NHWC strides")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child == "direct":
        return child_direct(a)
    m = back2future.Model("random:hard:2:1.0")
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    res = {"metric": "conv3x3 backward", "n": a.n, "H": a.height, "W": a.width, "layout": a.layout, "reps": a.reps, "layers": {}}
    for ci, co in LAYERS:
        x, w, b, gy = layer_data(ci, co, a.n, a.height, a.width)
        y, fwd = forward_row(m, x, w, b, a.reps)
        _, rows = row_medians(m, lambda: ops.conv3x3_backward(m, x, w, gy, y=y, leaky=True, layout=a.layout), a.reps)
        conv = [k for k in rows if k.startswith("conv") and not k.startswith("convbwd_")]
        assert len(conv) == 1, rows
        partials, chain = ops.conv3x3_backward_plan(m, a.n, ci, a.height, a.width, co)
        flop = 2.0 * 9 * ci * co * a.n * a.height * a.width
        gw = rows["convbwd_gradw"] + rows["convbwd_reduce"]
        res["layers"]["%dto%d" % (ci, co)] = {
            "gradinput": {"row": conv[0], "ms": round(rows[conv[0]], 4)}, "mask_ms": round(rows["convbwd_mask"], 4),
            "gradw_ms": round(rows["convbwd_gradw"], 4), "reduce_ms": round(rows["convbwd_reduce"], 4), "gradw_reduce_ms": round(gw, 4),
            "partials": partials, "longest_chain": chain, "forward_default": fwd, "flop": flop,
            "gradw_tflops": round(flop / (gw * 1e-3) / 1e12, 2), "gradw_share_of_peak": round(flop / (gw * 1e-3) / FP32_MATRIX_PEAK, 4)}
    m.close()
    # the direct kernel is chosen by the environment, read once per process: a fresh child, one at a time, under a time limit
    env = dict(os.environ, B2F_WINO="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "direct", "--n", str(a.n), "--height", str(a.height), "--width", str(a.width),
           "--reps", str(a.reps)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit("the child that times the direct kernel failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-2000:]))
    direct = json.loads(p.stdout.strip().splitlines()[-1])
    for key, row in direct.items():
        L = res["layers"][key]
        L["forward_direct"] = row
        L["gradw_over_forward_direct"] = round(L["gradw_reduce_ms"] / row["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
