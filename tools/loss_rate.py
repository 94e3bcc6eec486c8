"""What the unsupervised validation loss (test.lua:266-297) costs on the GPU (GPU box only): Model.forwardLoss, which reduces the
output table on the device, against Model.forward, which downloads it, and the loss kernels against their byte floor.

    python tools/loss_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--model random:soft:2:1.0]

Prints ONE JSON line; every timing row is the median of `reps` calls with its minimum and maximum:
  forward        Model.forward(x): the table (20 or 25 tensors) comes down the link
  forward_loss   Model.forwardLoss(x): n x L x 128 bytes come down
  table_mb       the size of the table per triplet
  equal          forwardLoss's words equal ops.table_loss (host entry) of forward's table
  kernel         the loss stage's time per call from option profile = 1 (the row "table_loss": HIP events around the memset, the
                 pooling passes and the L loss launches), the bytes it has to move -- computed from the shapes here: per pixel of every
                 level 13 (Hard) or 15 (Soft) floats read once, plus the pooling passes' 3 floats read at level j and 3 written at
                 level j + 1 -- and what that is in bytes/s against the 6.29 TB/s a float4 copy reaches on this chip
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
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", default="random:soft:2:1.0")
    a = ap.parse_args()
    n, H, W = a.n, a.height, a.width
    m = back2future.Model(a.model)
    L = m.n_outputs // (5 if m.past_flow else 4)
    res = {"metric": "table loss", "n": n, "H": H, "W": W, "model": a.model, "levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    out = [None, None]

    def fwd():
        out[0] = m.forward(x)

    def fwd_loss():
        out[1] = m.forwardLoss(x)

    res["forward"] = stats(host_ms(fwd, a.reps))
    res["forward_loss"] = stats(host_ms(fwd_loss, a.reps))
    res["table_mb"] = round(sum(t.nbytes for t in out[0]) / n / 1e6, 1)
    res["equal"] = bool(np.array_equal(out[1], ops.table_loss(out[0], x[:, 3:6])))
    # the kernels alone: bytes from the shapes
    floats = 15 if m.past_flow else 13
    level_px = [(H >> j) * (W >> j) for j in range(L)]
    nbytes = n * 4 * (sum(floats * p for p in level_px) + sum(3 * level_px[j] + 3 * level_px[j + 1] for j in range(L - 1)))
    m.set_option("profile", 1)
    m.forwardLoss(x)
    m.profile_reset()
    for _ in range(a.reps):
        m.forwardLoss(x)
    rows = m.profile_read()
    m.set_option("profile", 0)
    ms, launches = rows["table_loss"]
    per_call = ms / max(launches, 1)
    res["kernel"] = {"ms_per_call": round(per_call, 4), "calls": launches, "bytes": nbytes, "bytes_per_px_level0": floats * 4,
                     "tb_per_s": round(nbytes / (per_call * 1e-3) / 1e12, 3), "share_of_copy_rate": round(nbytes / (per_call * 1e-3) / 1e12 / HBM_COPY_TB_S, 3)}
    res["summary_mean"] = back2future.loss_summary(out[1])["mean"]
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
