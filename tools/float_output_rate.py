"""Triplets/s of computeFlow's float64 and float32 output paths on a video clip (GPU box only).

    python tools/float_output_rate.py [--frames 18] [--sizes 1024x1920,1080x1920] [--host-reps 5] [--steps 20]

The frames are tools/sequence_rate.py's clip() (18 u8 frames: 16 triplets), random Hard weights, library defaults.  For each
size, median milliseconds per call (host rows) or mean over --steps calls (device row), and the bytes of output per triplet:
  seq_f64           computeFlowSequence(V) on the u8 host frames, float64 flow (sequence_rate.py row d)
  seq_f32           the same with dtype=np.float32, pageable output buffers
  seq_f32_pinned    dtype=np.float32 into page-locked output buffers (DMA'd in place)
  seq_f32_occ       dtype=np.float32, occ_prob=True, pageable buffers
  seq_device_u8     b2f_compute_flow_sequence_device on the u8 frames in device memory (flow, occ_prob and masks)
  batch_f64         computeFlowBatch(V[:-2], V[1:-1], V[2:]) on the same bytes, float64 flow
  batch_f32         the same with dtype=np.float32, pageable buffers
Prints ONE JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from back2future_amd import back2future

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sequence_rate import clip, time_device, time_host   # noqa: E402


def rows_for(m, T, H, W, a):
    B = T - 2
    V = clip(T, H, W, seed=2)
    Vn = V.numpy()
    px = H * W
    f64 = (np.empty((B, 2, H, W), np.float64), np.empty((B, 1, H, W), np.uint8), np.empty((B, 1, H, W), np.uint8))
    f32 = (np.empty((B, 2, H, W), np.float32), np.empty((B, 1, H, W), np.uint8), np.empty((B, 1, H, W), np.uint8))
    occ = np.empty((B, 2, H, W), np.float32)
    pin = tuple(t.pin_memory().numpy() for t in (torch.empty((B, 2, H, W)), torch.empty((B, 1, H, W), dtype=torch.uint8),
                                                  torch.empty((B, 1, H, W), dtype=torch.uint8)))
    ms, path, out_bytes = {}, {}, {}
    ms["seq_f64"] = time_host(lambda: m.computeFlowSequence(Vn, out=f64), a.host_reps)
    ms["seq_f32"] = time_host(lambda: m.computeFlowSequence(Vn, dtype=np.float32, out=f32), a.host_reps)
    ms["seq_f32_pinned"] = time_host(lambda: m.computeFlowSequence(Vn, dtype=np.float32, out=pin), a.host_reps)
    ms["seq_f32_occ"] = time_host(lambda: m.computeFlowSequence(Vn, dtype=np.float32, occ_prob=True, out=f32 + (occ,)), a.host_reps)
    d_u8 = V.cuda()
    d_out = (torch.empty((B, 2, H, W), device="cuda"), torch.empty((B, 2, H, W), device="cuda"),
             torch.empty((B, 1, H, W), dtype=torch.uint8, device="cuda"), torch.empty((B, 1, H, W), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    ms["seq_device_u8"] = time_device(m, lambda: m.computeFlowSequenceDevice(d_u8.data_ptr(), T, H, W, *[t.data_ptr() for t in d_out],
                                                                             in_kind=back2future.IN_U8), a.steps)
    ms["batch_f64"] = time_host(lambda: m.computeFlowBatch(Vn[:-2], Vn[1:-1], Vn[2:], out=f64), a.host_reps)
    ms["batch_f32"] = time_host(lambda: m.computeFlowBatch(Vn[:-2], Vn[1:-1], Vn[2:], dtype=np.float32, out=f32), a.host_reps)
    for k in ms:
        out_bytes[k] = px * (2 * 8 + 2 if k.endswith("f64") else 2 * 4 + 2 + (2 * 4 if k in ("seq_f32_occ", "seq_device_u8") else 0))
    path.update(seq_f64="computeFlowSequence, u8 host frames, f64 flow", seq_f32="computeFlowSequence dtype=float32, pageable outputs",
                seq_f32_pinned="computeFlowSequence dtype=float32, pinned outputs", seq_f32_occ="computeFlowSequence dtype=float32 occ_prob=True, pageable outputs",
                seq_device_u8="computeFlowSequenceDevice, u8 device frames, flow + occ_prob + masks", batch_f64="computeFlowBatch, u8 host views, f64 flow",
                batch_f32="computeFlowBatch dtype=float32, u8 host views, pageable outputs")
    return {k: {"ms": round(v, 3), "triplets_per_s": round(B * 1e3 / v, 1), "out_bytes_per_triplet": out_bytes[k], "path": path[k]}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18)
    ap.add_argument("--sizes", default="1024x1920,1080x1920")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    m = back2future.Model("random:hard:2:1.0")
    res = {"metric": "float32 vs float64 computeFlow outputs", "frames": a.frames, "triplets": a.frames - 2, "model": "random:hard:2:1.0",
           "sizes": {}}
    for s in a.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        rows = rows_for(m, a.frames, H, W, a)
        res["sizes"][s] = {"rows": rows,
                           "seq_f32_over_f64": round(rows["seq_f64"]["ms"] / rows["seq_f32"]["ms"], 4),
                           "seq_f32_pinned_over_f64": round(rows["seq_f64"]["ms"] / rows["seq_f32_pinned"]["ms"], 4),
                           "batch_f32_over_f64": round(rows["batch_f64"]["ms"] / rows["batch_f32"]["ms"], 4)}
        torch.cuda.empty_cache()
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
