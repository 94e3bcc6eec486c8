"""What the occlusion-aware SSIM + L1 photometric term (criterions/OSSIML1Criterion.lua; words 16 .. 25 of the 32-word records) costs
on the GPU (GPU box only): Model.forwardLoss(objective="ssim", ssim_range="image") against Model.forwardLoss in the same run, and the
two new stages against the existing loss stage and against their byte floor.

    python tools/loss_ssim_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--models random:hard:2:1.0,random:soft:2:1.0]

Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum and maximum:
  forward_loss       Model.forwardLoss(x): n x L x 128 bytes come down
  forward_loss_ssim  Model.forwardLoss(x, objective="ssim", ssim_range="image"): n x L x 256 bytes come down
  equal_words_0_15   words 0 .. 15 of the 32-word records equal the 16-word records
  equal_host         the 32-word records of the first triplet equal ops.table_loss(objective="ssim", ssim_range="image") (host entry) of
                     forward's table
  table_loss         the existing stage's time per call from option profile = 1 inside the SSIM call (the memset of the wider
                     records, the pooling passes and the L launches of table_loss_kernel)
  table_loss_range   the range stage's time per call (L launches of table_loss_range_kernel and the one that combines them) and the
                     bytes it has to move: the nine planes of every level, read once
  table_loss_ssim    the SSIM stage's time per call (the L launches of table_loss_ssim_kernel), the bytes it has to move -- the same
                     nine planes, the flow of each direction (2 planes for a Hard table, 4 for a Soft one) and the two occlusion planes,
                     read once; the halo rows and columns and the second read of the centre values are re-reads that the cache can
                     serve -- what that is in bytes/s against the 6.29 TB/s a float4 copy reaches on this chip
  ratio_to_table_loss  (table_loss_range + table_loss_ssim) / table_loss of the same run
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


def measure(model, n, H, W, reps, check):
    m = back2future.Model(model)
    L = m.n_outputs // (5 if m.past_flow else 4)
    res = {"levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    out = [None, None]

    def fwd_loss():
        out[0] = m.forwardLoss(x)

    def fwd_loss_ssim():
        out[1] = m.forwardLoss(x, objective="ssim", ssim_range="image")

    res["forward_loss"] = stats(host_ms(fwd_loss, reps))
    res["forward_loss_ssim"] = stats(host_ms(fwd_loss_ssim, reps))
    res["equal_words_0_15"] = bool(np.array_equal(out[1][:, :, :16], out[0]))
    if check:   # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
        table = [t[:1] for t in m.forward(x)]
        res["equal_host"] = bool(np.array_equal(out[1][:1], ops.table_loss(table, x[:1, 3:6], objective="ssim", ssim_range="image")))
    level_px = [(H >> j) * (W >> j) for j in range(L)]
    nbytes_range = n * 4 * sum(9 * p for p in level_px)
    nbytes_ssim = n * 4 * sum((9 + (4 if m.past_flow else 2) + 2) * p for p in level_px)
    nbytes = n * 4 * sum((15 if m.past_flow else 13) * p for p in level_px) + n * 4 * sum(3 * level_px[j] + 3 * level_px[j + 1] for j in range(L - 1))
    m.set_option("profile", 1)
    m.forwardLoss(x, objective="ssim", ssim_range="image")
    m.profile_reset()
    for _ in range(reps):
        m.forwardLoss(x, objective="ssim", ssim_range="image")
    rows = m.profile_read()
    m.set_option("profile", 0)

    def row(name, b):
        ms, launches = rows[name]
        per_call = ms / max(launches, 1)
        return {"ms_per_call": round(per_call, 4), "calls": launches, "bytes": b, "tb_per_s": round(b / (per_call * 1e-3) / 1e12, 3),
                "share_of_copy_rate": round(b / (per_call * 1e-3) / 1e12 / HBM_COPY_TB_S, 3)}

    res["table_loss"] = row("table_loss", nbytes)
    res["table_loss_range"] = row("table_loss_range", nbytes_range)
    res["table_loss_ssim"] = row("table_loss_ssim", nbytes_ssim)
    res["ratio_to_table_loss"] = round((res["table_loss_range"]["ms_per_call"] + res["table_loss_ssim"]["ms_per_call"]) / res["table_loss"]["ms_per_call"], 3)
    res["profile_rows"] = dict((k, [round(v[0] / max(v[1], 1), 4), v[1]]) for k, v in rows.items())
    res["summary_mean"] = back2future.loss_summary(out[1], pme_criterion="OSSIML1")["mean"]
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="random:hard:2:1.0,random:soft:2:1.0")
    ap.add_argument("--no-host-check", action="store_true", help="skip the host entry on one triplet (seconds of CPU at full HD)")
    a = ap.parse_args()
    res = {"metric": "table loss ssim", "n": a.n, "H": a.height, "W": a.width}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps, not a.no_host_check)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
