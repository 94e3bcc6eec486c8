"""What the Soft models' past flow costs (GPU box only): the pruned forward pass and the float32 host entry with and without it, the
full table of Model.forward that was the only way to it before, and the warp stage with and without the own past flow.

    python tools/past_flow_rate.py [--triplets 16] [--height 1024] [--width 1920] [--reps 5] [--parent-root DIR] [--out FILE]

Prints ONE JSON line; every row is the median of `reps` calls with its minimum and maximum (ms per call, and per triplet):
  forward_device        Model.forward_device on `triplets` byte triplets (as [0, 1] floats on the GPU), use_graph = 1
  forward_device_past   the same with d_past_flow: five more 6-layer decoders, four more x2 upsamplings
  f32_host              Model.computeFlowBatch(dtype=float32) on the byte triplets from pageable host memory
  past_host             Model.computeFlowBatchPast on the same: 8 B/px more come down the link
  forward_table         Model.forward at n = 4 (the whole 25-tensor table downloaded), the only way to the past flow before
  forward_device_past_n4  forward_device_past at the same n = 4: must be faster per triplet than forward_table (the margin is that
                        row's own spread: its minimum against this row's maximum)
  past_chain            what the past chain costs over forward_device: ms per triplet and the share of a step
  warp_stage            the profile row "flow_warp" of computeFlowBatchWarp(want_warped=False) per call, with own_past_flow and without
--parent-root DIR: a built checkout of the parent commit; forward_device and f32_host are measured there too, by this tool in a
process of its own (--only-parent-rows --root DIR), and `parent_within_spread` says whether this commit's medians lie inside the
parent's minimum .. maximum widened by this commit's own spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

# --root DIR: import the package from another checkout (the parent commit's)
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from back2future_amd import back2future

MODEL = "random:soft:2:1.0"


def row(ms, n):
    med = statistics.median(ms)
    return {"ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "ms_per_triplet": round(med / n, 4),
            "triplets_per_s": round(n * 1e3 / med, 1)}


def timed(m, call, reps, warm=3, device=True):
    """ms of each of `reps` calls after `warm` (eager, capture, replay)"""
    for _ in range(warm):
        call()
    m.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        if device:
            m.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triplets", type=int, default=16)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--only-parent-rows", action="store_true", help="forward_device and f32_host alone: the calls a parent commit can run")
    a = ap.parse_args()
    n, H, W, reps = a.triplets, a.height, a.width, a.reps
    m = back2future.Model(MODEL)
    r = np.random.default_rng(2)
    ims = [r.integers(0, 256, (n, 3, H, W), dtype=np.uint8) for _ in range(3)]
    x = torch.from_numpy(np.concatenate(ims, axis=1)).cuda().float().div_(255.0).contiguous()   # n x 9 x H x W in [0, 1]
    dev = lambda *s: torch.empty(s, device="cuda")
    flow, occ, est3, past = dev(n, 2, H, W), dev(n, 2, H, W), dev(n, 2, H, W), dev(n, 2, H, W)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    res = {"metric": "past flow", "triplets": n, "H": H, "W": W, "model": MODEL, "reps": reps, "rows": {}}
    R = res["rows"]
    f32_out = (np.empty((n, 2, H, W), np.float32), np.empty((n, 1, H, W), np.uint8), np.empty((n, 1, H, W), np.uint8))
    with m.options(use_graph=1):
        R["forward_device"] = row(timed(m, lambda: m.forward_device(p(x), n, H, W, p(flow), p(occ), p(est3), unit_input=True), reps), n)
    R["f32_host"] = row(timed(m, lambda: m.computeFlowBatch(*ims, dtype=np.float32, out=f32_out), reps, warm=2, device=False), n)
    if a.only_parent_rows:
        print(json.dumps(res))
        m.close()
        return
    with m.options(use_graph=1):
        R["forward_device_past"] = row(timed(m, lambda: m.forward_device(p(x), n, H, W, p(flow), p(occ), p(est3), unit_input=True,
                                                                          d_past_flow=p(past)), reps), n)
        n4 = min(4, n)
        R["forward_device_past_n4"] = row(timed(m, lambda: m.forward_device(p(x), n4, H, W, p(flow), p(occ), p(est3), unit_input=True,
                                                                             d_past_flow=p(past)), reps), n4)
    past_out = (f32_out[0], np.empty((n, 2, H, W), np.float32), f32_out[1], f32_out[2])
    R["past_host"] = row(timed(m, lambda: m.computeFlowBatchPast(*ims, out=past_out), reps, warm=2, device=False), n)
    xn = x[:n4].cpu().numpy()   # (Model.forward takes normalized input; the time does not depend on the values)
    R["forward_table"] = row(timed(m, lambda: m.forward(xn), reps, warm=1, device=False), n4)
    res["past_faster_than_table"] = bool(R["forward_device_past_n4"]["max_ms"] < R["forward_table"]["min_ms"])
    extra = R["forward_device_past"]["ms"] - R["forward_device"]["ms"]
    res["past_chain"] = {"ms_per_triplet": round(extra / n, 4), "share_of_forward_device": round(extra / R["forward_device"]["ms"], 4)}
    # ---- the warp stage alone: the profile row of the same call (profiling runs the forward pass eagerly; the row is the stage's own)
    photo = np.empty((n, 14), np.uint64)
    res["warp_stage"] = {}
    for name, own in (("plain", False), ("own_past_flow", True)):
        per = []
        with m.options(profile=1):
            for _ in range(reps):
                m.profile_reset()
                m.computeFlowBatchWarp(*ims, want_warped=False, out=photo, own_past_flow=own)
                per.append(m.profile_read()["flow_warp"][0])
        res["warp_stage"][name] = {"ms_per_call": round(statistics.median(per), 4), "min_ms": round(min(per), 4), "max_ms": round(max(per), 4)}
    if a.parent_root:
        q = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-parent-rows", "--root", a.parent_root, "--triplets", str(n),
                            "--height", str(H), "--width", str(W), "--reps", str(reps)], capture_output=True, text=True)
        if q.returncode != 0:
            sys.exit("the rows on the parent checkout failed:\n" + q.stdout + q.stderr)
        P = json.loads(q.stdout.strip().splitlines()[-1])["rows"]
        res["on_parent_commit"] = P
        within = {}
        for k in ("forward_device", "f32_host"):
            spread = R[k]["max_ms"] - R[k]["min_ms"]
            within[k] = bool(P[k]["min_ms"] - spread <= R[k]["ms"] <= P[k]["max_ms"] + spread)
        res["parent_within_spread"] = within
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
