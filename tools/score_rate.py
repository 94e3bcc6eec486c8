"""What scoring against ground truth costs (GPU box only): computeFlowBatchScore against the float32 entry followed by the host's numpy
scoring, and the score kernel alone.

    python tools/score_rate.py [--triplets 16] [--height 1024] [--width 1920] [--reps 5] [--numpy-reps 1]

Prints ONE JSON line:
  gpu_score     Model.computeFlowBatchScore (uint8 frames, ground-truth flow + valid + gt_occ, pageable buffers), median of `reps` calls:
                ms and triplets/s; 176 bytes per triplet come down the link
  f32_only      Model.computeFlowBatch(dtype=float32, occ_prob=True) alone, the same way: 10 + 8 B/px come down
  numpy_score   the fp64 numpy scoring of tests/flow_score_fields.py on that call's outputs: seconds for the n images, and
                f32_plus_numpy: triplets/s of the two together
  equal         the GPU's words equal the numpy restatement's
  kernel        the score stage's time per call from option profile = 1 (the row "flow_score": HIP events around the launch and its
                memset), and what that is in bytes/s at 26 B/px against the 6.29 TB/s a float4 copy reaches on this chip
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from back2future_amd import back2future
from tests import flow_score_fields as F
from tools.sequence_rate import clip

HBM_COPY_TB_S = 6.29


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
    ap.add_argument("--triplets", type=int, default=16)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-reps", type=int, default=1)
    a = ap.parse_args()
    n, H, W = a.triplets, a.height, a.width
    m = back2future.Model("random:soft:2:1.0")
    res = {"metric": "flow scores", "triplets": n, "H": H, "W": W, "model": "random:soft:2:1.0"}
    V = clip(n + 2, H, W, seed=2).numpy()
    ims = [np.ascontiguousarray(x) for x in (V[:-2], V[1:-1], V[2:])]
    f32_out = (np.empty((n, 2, H, W), np.float32), np.empty((n, 1, H, W), np.uint8), np.empty((n, 1, H, W), np.uint8),
               np.empty((n, 2, H, W), np.float32))
    flow, _, _, prob = m.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True, out=f32_out)
    r = np.random.default_rng(3)
    gt = (flow * np.float32(20.0) + r.normal(0, 2.0, flow.shape).astype(np.float32)).astype(np.float32)
    valid = (r.random((n, H, W)) < 0.9).astype(np.uint8)
    occ = r.choice(np.array([0, 1, 1, 1, 2], np.uint8), (n, H, W))
    scores = np.empty((n, 22), np.uint64)

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    res["gpu_score"] = stats(host_ms(lambda: m.computeFlowBatchScore(*ims, gt, valid=valid, gt_occ=occ, out=scores), a.reps))
    f32_ms = host_ms(lambda: m.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True, out=f32_out), a.reps)
    res["f32_only"] = stats(f32_ms)
    np_s = []
    for _ in range(a.numpy_reps):
        t0 = time.perf_counter()
        want = F.numpy_scores(flow, gt, occ_prob=prob, valid=valid, gt_occ=occ)
        np_s.append(time.perf_counter() - t0)
    np_med = statistics.median(np_s)
    both_ms = statistics.median(f32_ms) + np_med * 1e3
    res["numpy_score"] = {"s": round(np_med, 3), "ms_per_triplet": round(np_med * 1e3 / n, 2)}
    res["f32_plus_numpy"] = {"ms": round(both_ms, 1), "triplets_per_s": round(n * 1e3 / both_ms, 2)}
    res["speedup"] = round(both_ms / res["gpu_score"]["ms"], 1)
    res["equal"] = bool(np.array_equal(scores, want))
    res["summary"] = {k: (None if v != v else v) for k, v in back2future.score_summary(scores).items()}

    # ---- the score stage alone: the profile row of the same call (profiling runs the forward pass eagerly; the row is the stage's own)
    with m.options(profile=1):
        m.profile_reset()
        calls = 3
        for _ in range(calls):
            m.computeFlowBatchScore(*ims, gt, valid=valid, gt_occ=occ, out=scores)
        ms, launches = m.profile_read()["flow_score"]
    per_call = ms / calls
    px = n * H * W
    tb_s = px * 26 / (per_call * 1e-3) / 1e12
    res["kernel"] = {"ms_per_call": round(per_call, 4), "launches_per_call": launches // calls, "bytes_per_px": 26, "TB_per_s": round(tb_s, 3),
                     "share_of_hbm_copy_rate": round(tb_s / HBM_COPY_TB_S, 3), "hbm_copy_TB_per_s": HBM_COPY_TB_S}
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
