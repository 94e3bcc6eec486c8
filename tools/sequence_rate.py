"""Triplets/s of a video clip run as overlapping triplets against the same clip run as a sequence (GPU box only).

    python tools/sequence_rate.py [--frames 18] [--height 1024] [--width 1920] [--steps 20] [--layers OUT.json]

18 frames -> 16 triplets (the bench's batch) at 1024 x 1920, random Hard weights, library defaults; the device rows write the
bench's outputs (flow, occ, est[3]).  Prints ONE JSON line:
  a  forward_device on the T-2 overlapping triplets (T-2 x 9 x H x W, [0,1] floats), use_graph = 1
  b  forward_sequence_device on the T frames (T x 3 x H x W, the same floats), use_graph = 1
  b_u8  the same from the 8-bit frames (in_kind = IN_U8; extra row)
  c  computeFlowBatch(V[:-2], V[1:-1], V[2:]) on the uint8 host frames (views, no copies)
  d  computeFlowSequence(V) on the same bytes
with b/a and d/c.  --layers writes the profile_layers = 1 rows (ms per forward) of (a) and (b) to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from back2future_amd import back2future


def clip(T, H, W, seed):
    """T frames of a scene panning by (+3, +1) px per frame, plus U(-0.02, 0.02) noise (the bench's synthetic triplets,
    continued): T x 3 x H x W in [0, 1], quantised to bytes."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, 3, H + 4 * T + 8, W + 4 * T + 8, generator=g)
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0]
    out = torch.empty(T, 3, H, W)
    for t in range(T):
        out[t] = base[:, 4 + t:4 + t + H, 4 + 3 * t:4 + 3 * t + W] + (torch.rand(3, H, W, generator=g) - 0.5) * 0.04
    return (out.clamp_(0, 1) * 255).round_().to(torch.uint8)


def time_device(m, call, steps):
    for _ in range(3):           # eager, capture, first replay
        call()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def time_host(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def layer_rows(m, call):
    with m.options(profile=1, profile_layers=1):
        call()
        m.synchronize()
        m.profile_reset()
        call()
        m.synchronize()
        rows = {k: round(v[0], 4) for k, v in m.profile_read().items()}
        m.profile_reset()
    return dict(sorted(rows.items(), key=lambda kv: -kv[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--layers", default=None)
    a = ap.parse_args()
    T, H, W = a.frames, a.height, a.width
    B = T - 2
    m = back2future.Model("random:hard:2:1.0")
    V = clip(T, H, W, seed=2)
    d_u8 = V.cuda()
    d_seq = (d_u8.float() / 255).contiguous()
    d_tri = torch.cat([d_seq[:-2], d_seq[1:-1], d_seq[2:]], dim=1).contiguous()
    flow = torch.empty(B, 2, H, W, device="cuda")
    occ = torch.empty(B, 2, H, W, device="cuda")
    est3 = torch.empty(B, 3, H, W, device="cuda")
    torch.cuda.synchronize()
    run_a = lambda: m.forward_device(d_tri.data_ptr(), B, H, W, flow.data_ptr(), occ.data_ptr(), est3.data_ptr(), unit_input=True)
    run_b = lambda: m.forward_sequence_device(d_seq.data_ptr(), T, H, W, flow.data_ptr(), occ.data_ptr(), est3.data_ptr(), in_kind=back2future.IN_UNIT)
    run_bu = lambda: m.forward_sequence_device(d_u8.data_ptr(), T, H, W, flow.data_ptr(), occ.data_ptr(), est3.data_ptr(), in_kind=back2future.IN_U8)
    res = {"metric": "sequence vs overlapping triplets", "frames": T, "triplets": B, "H": H, "W": W, "model": "random:hard:2:1.0"}
    with m.options(use_graph=1):
        ms = {"a": time_device(m, run_a, a.steps), "b": time_device(m, run_b, a.steps), "b_u8": time_device(m, run_bu, a.steps)}
    Vn = V.numpy()
    out = tuple(np.empty(s, dt) for s, dt in (((B, 2, H, W), np.float64), ((B, 1, H, W), np.uint8), ((B, 1, H, W), np.uint8)))
    ms["c"] = time_host(lambda: m.computeFlowBatch(Vn[:-2], Vn[1:-1], Vn[2:], out=out), a.host_reps)
    ms["d"] = time_host(lambda: m.computeFlowSequence(Vn, out=out), a.host_reps)
    rows = {k: {"ms": round(v, 3), "triplets_per_s": round(B * 1e3 / v, 1)} for k, v in ms.items()}
    rows["a"]["path"] = "forward_device, %d x 9 x H x W f32, use_graph=1" % B
    rows["b"]["path"] = "forward_sequence_device, %d x 3 x H x W f32, use_graph=1" % T
    rows["b_u8"]["path"] = "forward_sequence_device, %d x 3 x H x W u8 (IN_U8), use_graph=1" % T
    rows["c"]["path"] = "computeFlowBatch on u8 host views"
    rows["d"]["path"] = "computeFlowSequence on the same u8 host frames"
    res["rows"] = rows
    res["b_over_a"] = round(ms["a"] / ms["b"], 4)
    res["b_u8_over_a"] = round(ms["a"] / ms["b_u8"], 4)
    res["d_over_c"] = round(ms["c"] / ms["d"], 4)
    if a.layers:
        lay = {"a": layer_rows(m, run_a), "b": layer_rows(m, run_b), "b_u8": layer_rows(m, run_bu)}
        lay["totals_ms"] = {k: round(sum(v.values()), 3) for k, v in list(lay.items())}
        with open(a.layers, "w") as f:
            json.dump(lay, f, indent=1)
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
