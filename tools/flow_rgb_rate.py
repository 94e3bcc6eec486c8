"""What flow pictures cost (GPU box only): the xy2rgb kernels alone, and computeFlowSequenceRGB against the float32 entry.

    python tools/flow_rgb_rate.py [--frames 18] [--height 1024] [--width 1920] [--launches 20] [--host-reps 5]

Prints ONE JSON line:
  kernel     b2f_flow_rgb_device on a (frames - 2) x 2 x H x W float32 flow in device memory, mean of `launches` launches after
             warm-up: fixed max (reads 8, writes 3 B/px) and automatic max (the norm-max kernel reads the flow once more: 19 B/px),
             planar and packed, with the bytes/s each achieves
  host       sequence_rate.py's clip (uint8 frames, Hard model, library defaults), median of `host-reps` calls each:
             seq_f32 (flow + masks, pageable), seq_rgb_only, seq_rgb_flow_masks, seq_rgb_only_pinned; the spread (max - min) of
             the seq_f32 calls is the margin of "seq_rgb_only is no slower than seq_f32"
  host_xy2rgb_s  flow_io.xy2rgb on one H x W field, once, times the triplets: the host colouring the call replaces
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

from back2future_amd import back2future, flow_io
from tools.sequence_rate import clip


def host_ms(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    T, H, W = a.frames, a.height, a.width
    n = T - 2
    px = n * H * W
    m = back2future.Model("random:hard:2:1.0")
    res = {"metric": "flow pictures", "frames": T, "triplets": n, "H": H, "W": W, "model": "random:hard:2:1.0"}

    # ---- the kernels alone: a smooth field of up to ~30 px, the colours of a real picture
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    one = torch.stack([30 * torch.sin(xx / 97) * torch.cos(yy / 61), 12 * torch.cos(xx / 45)]) + torch.randn(2, H, W, generator=g) * 2
    d_flow = (one[None] * torch.linspace(0.5, 1.5, n)[:, None, None, None]).contiguous().cuda()
    d_rgb = torch.empty(n * 3 * H * W, dtype=torch.uint8, device="cuda")
    d_max = torch.empty(n, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    kernel = {}
    for name, mx, packed, bpp in (("fixed_planar", 20.0, False, 11), ("fixed_packed", 20.0, True, 11), ("auto_planar", None, False, 19),
                                  ("auto_packed", None, True, 19)):
        call = lambda: m.flowRGBDevice(d_flow.data_ptr(), n, H, W, d_rgb.data_ptr(), max=mx, packed=packed, d_max_used=d_max.data_ptr(),
                                       stream=stream.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.launches):
                call()
            e1.record(stream)
        stream.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.launches
        kernel[name] = {"us": round(us, 1), "bytes_per_px": bpp, "TB_per_s": round(px * bpp / us / 1e6, 3)}
    res["kernel"] = kernel
    del d_flow, d_rgb, d_max
    torch.cuda.empty_cache()

    # ---- the host entries on sequence_rate.py's clip
    V = clip(T, H, W, seed=2).numpy()
    f32_out = (np.empty((n, 2, H, W), np.float32), np.empty((n, 1, H, W), np.uint8), np.empty((n, 1, H, W), np.uint8))
    rgb_out = (np.empty((n, H, W, 3), np.uint8), np.empty(n, np.float64))
    all_out = rgb_out + f32_out
    pin_out = (torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory().numpy(), torch.empty(n, dtype=torch.float64).pin_memory().numpy())
    calls = {
        "seq_f32": lambda: m.computeFlowSequence(V, dtype=np.float32, out=f32_out),
        "seq_rgb_only": lambda: m.computeFlowSequenceRGB(V, packed=True, out=rgb_out),
        "seq_rgb_flow_masks": lambda: m.computeFlowSequenceRGB(V, packed=True, want_flow=True, want_masks=True, out=all_out),
        "seq_rgb_only_pinned": lambda: m.computeFlowSequenceRGB(V, packed=True, out=pin_out),
    }
    host = {}
    for name, call in calls.items():
        ms = host_ms(call, a.host_reps)
        med = statistics.median(ms)
        host[name] = {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
    res["host"] = host
    spread = host["seq_f32"]["max_ms"] - host["seq_f32"]["min_ms"]
    res["seq_f32_spread_ms"] = round(spread, 3)
    res["seq_rgb_only_no_slower"] = bool(host["seq_rgb_only"]["ms"] <= host["seq_f32"]["ms"] + spread)

    # ---- the host colouring the call replaces
    flow = f32_out[0][0]
    t0 = time.perf_counter()
    flow_io.xy2rgb(flow[0], flow[1])
    res["host_xy2rgb_s"] = round((time.perf_counter() - t0) * n, 3)
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
