"""What the fine-tuning objective of the Soft models (README.md:89-102; words 16 .. 23 of the 24-word records) costs on the GPU (GPU
box only): Model.forwardLoss(objective="finetune") against Model.forwardLoss in the same run, and the new stage against the
existing loss stage and against its byte floor.

    python tools/loss_ft_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--models random:hard:2:1.0,random:soft:2:1.0]

Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum and maximum:
  forward_loss      Model.forwardLoss(x): n x L x 128 bytes come down
  forward_loss_ft   Model.forwardLoss(x, objective="finetune"): n x L x 192 bytes come down
  equal_words_0_15  words 0 .. 15 of the 24-word records equal the 16-word records
  equal_host        the 24-word records of the first triplet equal ops.table_loss(objective="finetune") (host entry) of forward's table
  table_loss        the existing stage's time per call from option profile = 1 inside the fine-tuning call (the memset of the wider
                    records, the pooling passes and the L launches of table_loss_kernel)
  table_loss_ft     the new stage's time per call (the L launches of table_loss_ft_kernel), the bytes it has to move -- per pixel of
                    every level the same 13 (Hard) or 15 (Soft) floats read once; the halo rows and columns are re-reads that the
                    cache can serve -- what that is in bytes/s against the 6.29 TB/s a float4 copy reaches on this chip, and its
                    ratio to the table_loss row
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

    def fwd_loss_ft():
        out[1] = m.forwardLoss(x, objective="finetune")

    res["forward_loss"] = stats(host_ms(fwd_loss, reps))
    res["forward_loss_ft"] = stats(host_ms(fwd_loss_ft, reps))
    res["equal_words_0_15"] = bool(np.array_equal(out[1][:, :, :16], out[0]))
    if check:   # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
        table = [t[:1] for t in m.forward(x)]
        res["equal_host"] = bool(np.array_equal(out[1][:1], ops.table_loss(table, x[:1, 3:6], objective="finetune")))
    floats = 15 if m.past_flow else 13
    level_px = [(H >> j) * (W >> j) for j in range(L)]
    nbytes_ft = n * 4 * sum(floats * p for p in level_px)
    nbytes = nbytes_ft + n * 4 * sum(3 * level_px[j] + 3 * level_px[j + 1] for j in range(L - 1))
    m.set_option("profile", 1)
    m.forwardLoss(x, objective="finetune")
    m.profile_reset()
    for _ in range(reps):
        m.forwardLoss(x, objective="finetune")
    rows = m.profile_read()
    m.set_option("profile", 0)

    def row(name, b):
        ms, launches = rows[name]
        per_call = ms / max(launches, 1)
        return {"ms_per_call": round(per_call, 4), "calls": launches, "bytes": b, "tb_per_s": round(b / (per_call * 1e-3) / 1e12, 3),
                "share_of_copy_rate": round(b / (per_call * 1e-3) / 1e12 / HBM_COPY_TB_S, 3)}

    res["table_loss"] = row("table_loss", nbytes)
    res["table_loss_ft"] = row("table_loss_ft", nbytes_ft)
    res["table_loss_ft"]["ratio_to_table_loss"] = round(res["table_loss_ft"]["ms_per_call"] / res["table_loss"]["ms_per_call"], 3)
    res["summary_mean"] = back2future.loss_summary(out[1], objective="Ours-Soft-ft-KITTI" if m.past_flow else "Ours-Hard")["mean"]
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
    res = {"metric": "table loss ft", "n": a.n, "H": a.height, "W": a.width}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps, not a.no_host_check)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
