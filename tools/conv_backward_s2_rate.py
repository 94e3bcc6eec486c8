"""What the backward pass of a stride-2 conv layer costs on the GPU (GPU box only): ops.conv3x3s2_backward (csrc/b2f_convbwd.hip) on the six
pyramid layers 3 -> 16, 16 -> 32, 32 -> 64, 64 -> 96, 96 -> 128, 128 -> 192 at the map sizes of a 1024 x 1920 forward pass (inputs 1024 x
1920, 512 x 960, .. 32 x 60), batch 4, next to the forward layer on the same data and to gradInput by the zero-inserted route.

    python tools/conv_backward_s2_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--layout 1] [--layers 0,1,2,3,4,5]

Prints ONE JSON line.  Every time is a profile row of the op entry (device events around the launches, option profile = 1), the median
over `reps` calls after one warm-up call; the host staging of the entry is not in it.  Per layer:
  mask, gradx, gradw, reduce   rows convbwd_mask, convbwd_gradx_s2, convbwd_gradw (conv3x3_gradw + gradb_partials), convbwd_reduce;
                               partials, longest_chain: the plan
  forward_default       ops.conv3x3(stride 2) with LeakyReLU under the default options: row name and time
  forward_direct        the same in a child process with B2F_WINO=0 and bf16_conv = 0 (the direct fp32 MFMA kernel where the layer has
                        one): the yardstick of both kernels, same FLOP count, same instruction
  gradx_zero_inserted   gradInput by the route conv3x3s2_gradx replaces: g' written into the even pixels of a zero 2 Ho x 2 Wo map, then
                        ops.conv3x3_backward(want x) at stride 1 on it: its mask row and the forward kernel's row (the zero insertion
                        itself is done on the host and is in neither)
  *_tflops              2 * 9 * Ci * Co * B * Ho * Wo FLOP over the time
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

LAYERS = [(3, 16), (16, 32), (32, 64), (64, 96), (96, 128), (128, 192)]          # (Ci, Co); layer i reads the map at 1 / 2^i
FP32_MATRIX_PEAK = 157.3e12


def layer_size(a, i):
    return a.height >> i, a.width >> i


def layer_data(ci, co, n, H, W):
    r = np.random.default_rng([7, ci, co, n, H, W])
    x = r.standard_normal((n, ci, H, W), dtype=np.float32)
    w = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    gy = r.standard_normal((n, co, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=np.float32)
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


def forward_kernel_row(rows):
    conv = [k for k in rows if k.startswith("conv") and not k.startswith("convbwd_")]
    assert len(conv) == 1, rows
    return {"row": conv[0], "ms": round(rows[conv[0]], 4)}


def forward_row(m, x, w, b, reps):
    y, rows = row_medians(m, lambda: ops.conv3x3(m, x, w, b, 2, True), reps)
    return y, forward_kernel_row(rows)


def model():
    m = back2future.Model("random:hard:2:1.0")
    m.set_option("profile", 1)
    m.set_option("profile_layers", 1)
    return m


def child_direct(a):
    m = model()
    m.set_option("bf16_conv", 0)
    res = {}
    for i in a.layers:
        ci, co = LAYERS[i]
        x, w, b, _ = layer_data(ci, co, a.n, *layer_size(a, i))
        res["%dto%d" % (ci, co)] = forward_row(m, x, w, b, a.reps)[1]
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layout", type=int, default=1, help="1: the forward's chunk-planar strides, 0: NHWC strides")
    ap.add_argument("--layers", default="0,1,2,3,4,5")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    a.layers = [int(i) for i in a.layers.split(",")]
    if a.child == "direct":
        return child_direct(a)
    m = model()
    res = {"metric": "conv3x3 stride-2 backward", "n": a.n, "H": a.height, "W": a.width, "layout": a.layout, "reps": a.reps, "layers": {}}
    for i in a.layers:
        ci, co = LAYERS[i]
        H, W = layer_size(a, i)
        x, w, b, gy = layer_data(ci, co, a.n, H, W)
        Ho, Wo = gy.shape[2:]
        y, fwd = forward_row(m, x, w, b, a.reps)
        _, rows = row_medians(m, lambda: ops.conv3x3s2_backward(m, x, w, gy, y=y, leaky=True, layout=a.layout), a.reps)
        partials, chain = ops.conv3x3s2_backward_plan(m, a.n, ci, H, W, co)
        # the comparator: g' (here gy itself, no activation: the mask row is reported apart) on the even pixels of a zero map
        g0 = np.zeros((a.n, co, 2 * Ho, 2 * Wo), np.float32)
        g0[:, :, ::2, ::2] = gy
        x0 = np.zeros((a.n, ci, 2 * Ho, 2 * Wo), np.float32)
        _, zrows = row_medians(m, lambda: ops.conv3x3_backward(m, x0, w, g0, leaky=False, layout=a.layout, want=("x",)), a.reps)
        del g0, x0
        flop = 2.0 * 9 * ci * co * a.n * Ho * Wo
        gw = rows["convbwd_gradw"] + rows["convbwd_reduce"]
        gx = rows["convbwd_gradx_s2"]
        zero = forward_kernel_row(zrows)
        zero["mask_ms"] = round(zrows["convbwd_mask"], 4)
        res["layers"]["%dto%d" % (ci, co)] = {
            "input": [H, W], "mask_ms": round(rows["convbwd_mask"], 4), "gradx_ms": round(gx, 4), "gradw_ms": round(rows["convbwd_gradw"], 4),
            "reduce_ms": round(rows["convbwd_reduce"], 4), "gradw_reduce_ms": round(gw, 4), "partials": partials, "longest_chain": chain,
            "forward_default": fwd, "gradx_zero_inserted": zero, "flop": flop,
            "gradx_tflops": round(flop / (gx * 1e-3) / 1e12, 2), "gradw_tflops": round(flop / (gw * 1e-3) / 1e12, 2),
            "gradw_share_of_peak": round(flop / (gw * 1e-3) / FP32_MATRIX_PEAK, 4),
            "gradx_over_zero_inserted": round(gx / zero["ms"], 3)}
    m.close()
    # the direct kernel is chosen by the environment, read once per process: a fresh child, one at a time, under a time limit
    env = dict(os.environ, B2F_WINO="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "direct", "--n", str(a.n), "--height", str(a.height), "--width", str(a.width),
           "--reps", str(a.reps), "--layers", ",".join(str(i) for i in a.layers)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit("the child that times the direct kernel failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-2000:]))
    direct = json.loads(p.stdout.strip().splitlines()[-1])
    for key, row in direct.items():
        L = res["layers"][key]
        L["forward_direct"] = row
        L["gradw_over_forward_direct"] = round(L["gradw_reduce_ms"] / row["ms"], 3)
        L["gradx_over_forward_direct"] = round(L["gradx_ms"] / row["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
