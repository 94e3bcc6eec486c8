"""What the gradient table of the Soft models' fine-tuning objective (the *_grad_ft entries: SecondOrderSmoothnessCriterion and
OBGCCriterion in train.lua:428-468) costs on the GPU (GPU box only): the new stage against the first-order gradient stage of the same
run -- the same planes read and written, a narrower stencil -- and against its byte floor.

    python tools/loss_grad_ft_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--objective NAME]
                                      [--models random:hard:2:1.0,random:soft:2:1.0]

The options are those of back2future.loss_grad_ft_options(): both criteria with alpha = beta = gamma = 1, the most work; --objective
NAME takes those of a released model.  Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum
and maximum:
  forward_loss_grad_device     Model.forwardLossGradDevice with the first-order options and the 16-word records
  forward_loss_grad_ft_device  the same with the fine-tuning options and the 24-word records
  equal_host                   the gradient of the first triplet equals ops.table_loss_grad (host entry, same options) of forward's
                               table; checked before anything is timed, and nothing is reported without it
  equal_records                the records of the fine-tuning call equal forwardLoss(objective="finetune")'s
  table_loss_grad              the first-order stage's time per call from option profile = 1 (the L launches of table_loss_grad_kernel)
  table_loss_grad_ft           the new stage's time per call (the L launches of table_loss_grad_ft_kernel), the bytes it has to move --
                               per pixel of every level the 13 (Hard) or 15 (Soft) floats it reads once plus the 10 or 12 it writes;
                               the wider halo and the second read of the reference are re-reads that the cache can serve --, what that
                               is in bytes/s against the 6.29 TB/s a float4 copy reaches on this chip, and its ratio to the
                               table_loss_grad row
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


def same_bits(a, b):
    return all(x.shape == y.shape and not ((x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))).any() for x, y in zip(a, b))


def measure(model, n, H, W, reps, objective):
    import torch
    m = back2future.Model(model)
    L = m.n_outputs // (5 if m.past_flow else 4)
    res = {"levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)
    # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
    ft = back2future.loss_grad_ft_options(objective=objective)
    grad, rec = m.forwardLossGrad(x, options=ft)
    table = [t[:1] for t in m.forward(x)]
    res["equal_host"] = bool(same_bits([g[:1] for g in grad], ops.table_loss_grad(table, x[:1, 3:6], options=ft)))
    if not res["equal_host"]:
        m.close()
        return res
    res["equal_records"] = bool(np.array_equal(rec, m.forwardLoss(x, objective="finetune")))
    del grad, table

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    dx = torch.from_numpy(x).cuda()
    dg = [torch.empty((n,) + s, dtype=torch.float32, device="cuda") for s in m.output_shapes(H, W)]
    dl = torch.empty((n, L, 24), dtype=torch.int64, device="cuda")
    ptrs = [g.data_ptr() for g in dg]

    def on_device(options=None):
        m.forwardLossGradDevice(dx.data_ptr(), n, H, W, ptrs, d_loss=dl.data_ptr(), options=options)
        torch.cuda.synchronize()

    res["forward_loss_grad_device"] = stats(host_ms(on_device, reps))
    res["forward_loss_grad_ft_device"] = stats(host_ms(lambda: on_device(ft), reps))
    read, written = (15, 12) if m.past_flow else (13, 10)
    level_px = [(H >> j) * (W >> j) for j in range(L)]
    nbytes_grad = n * 4 * sum((read + written) * p for p in level_px)
    m.set_option("profile", 1)
    on_device()
    on_device(ft)
    m.profile_reset()
    for _ in range(reps):
        on_device()
        on_device(ft)
    rows = m.profile_read()
    m.set_option("profile", 0)

    def row(name, b):
        ms, launches = rows[name]
        per_call = ms / max(launches, 1)
        return {"ms_per_call": round(per_call, 4), "calls": launches, "bytes": b, "tb_per_s": round(b / (per_call * 1e-3) / 1e12, 3),
                "share_of_copy_rate": round(b / (per_call * 1e-3) / 1e12 / HBM_COPY_TB_S, 3)}

    res["table_loss_grad"] = row("table_loss_grad", nbytes_grad)
    res["table_loss_grad_ft"] = row("table_loss_grad_ft", nbytes_grad)
    res["table_loss_grad_ft"]["ratio_to_table_loss_grad"] = round(res["table_loss_grad_ft"]["ms_per_call"] / res["table_loss_grad"]["ms_per_call"], 3)
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objective", default=None)
    ap.add_argument("--models", default="random:hard:2:1.0,random:soft:2:1.0")
    a = ap.parse_args()
    res = {"metric": "table loss grad ft", "n": a.n, "H": a.height, "W": a.width, "objective": a.objective}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps, a.objective)
        if not res[model].get("equal_host"):
            sys.exit("%s: the gradient of the first triplet differs from the host entry's; nothing reported" % model)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
