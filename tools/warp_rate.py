"""What motion compensation costs (GPU box only): computeFlowSequenceWarp against the float32 sequence entry, alone and followed by
the host entry, and the warp kernel alone.

    python tools/warp_rate.py [--frames 18] [--height 1024] [--width 1920] [--reps 5]

Prints ONE JSON line; every row is the median of `reps` calls with its minimum and maximum:
  photo_only     Model.computeFlowSequenceWarp(want_warped=False) on uint8 frames: 112 bytes per triplet come down the link
  warped_photo   the same with the warped frames: 6 B/px + 112 bytes
  f32_only       Model.computeFlowSequence(dtype=float32, occ_prob=True): 10 + 8 B/px come down
  f32_plus_host  the same followed by ops.flow_warp(model=None) of its outputs on the CPU
  photo_only_no_slower   photo_only's median is at most f32_only's maximum (the margin is that row's own spread)
  equal          the GPU's bytes and words equal the host entry's
  kernel         the warp stage's time per call from option profile = 1 (the row "flow_warp": HIP events around the launch and its
                 memset) with warped frames + photo, and what that is in bytes/s at the compulsory 31 B/px (flow 8 + probabilities 8 +
                 reference 3 + two neighbours read once 6 + warped 6) against the 6.29 TB/s a float4 copy reaches on this chip
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from back2future_amd import back2future, ops
from tools.sequence_rate import clip

HBM_COPY_TB_S = 6.29
BYTES_PER_PX = 31


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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    T, H, W = a.frames, a.height, a.width
    n = T - 2
    m = back2future.Model("random:soft:2:1.0")
    res = {"metric": "flow warp", "frames": T, "triplets": n, "H": H, "W": W, "model": "random:soft:2:1.0"}
    V = clip(T, H, W, seed=2).numpy()
    ims = [np.ascontiguousarray(x) for x in (V[:-2], V[1:-1], V[2:])]
    f32_out = (np.empty((n, 2, H, W), np.float32), np.empty((n, 1, H, W), np.uint8), np.empty((n, 1, H, W), np.uint8),
               np.empty((n, 2, H, W), np.float32))
    warped, photo = np.empty((n, 2, 3, H, W), np.uint8), np.empty((n, 14), np.uint64)
    photo_alone = np.empty((n, 14), np.uint64)

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    photo_ms = host_ms(lambda: m.computeFlowSequenceWarp(V, want_warped=False, out=photo_alone), a.reps)
    f32_ms = host_ms(lambda: m.computeFlowSequence(V, dtype=np.float32, occ_prob=True, out=f32_out), a.reps)
    both_ms = host_ms(lambda: m.computeFlowSequenceWarp(V, out=(warped, photo)), a.reps)
    res["photo_only"], res["warped_photo"], res["f32_only"] = stats(photo_ms), stats(both_ms), stats(f32_ms)
    res["photo_only_no_slower"] = bool(statistics.median(photo_ms) <= max(f32_ms))
    flow, prob = f32_out[0], f32_out[3]
    host = [None]

    def f32_then_host():
        m.computeFlowSequence(V, dtype=np.float32, occ_prob=True, out=f32_out)
        host[0] = ops.flow_warp(flow, *ims, occ_prob=prob)

    res["f32_plus_host"] = stats(host_ms(f32_then_host, max(1, min(a.reps, 3))))
    res["equal"] = bool(np.array_equal(host[0][0], warped) and np.array_equal(host[0][1], photo) and np.array_equal(photo, photo_alone))
    res["summary"] = {k: (None if v != v else v) for k, v in back2future.photo_summary(photo).items()}

    # ---- the warp stage alone: the profile row of the same call (profiling runs the forward pass eagerly; the row is the stage's own)
    with m.options(profile=1):
        m.profile_reset()
        calls = 3
        for _ in range(calls):
            m.computeFlowSequenceWarp(V, out=(warped, photo))
        ms, launches = m.profile_read()["flow_warp"]
    per_call = ms / calls
    tb_s = n * H * W * BYTES_PER_PX / (per_call * 1e-3) / 1e12
    res["kernel"] = {"ms_per_call": round(per_call, 4), "launches_per_call": launches // calls, "bytes_per_px": BYTES_PER_PX,
                     "TB_per_s": round(tb_s, 3), "share_of_hbm_copy_rate": round(tb_s / HBM_COPY_TB_S, 3), "hbm_copy_TB_per_s": HBM_COPY_TB_S}
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
