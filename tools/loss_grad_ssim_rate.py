"""What the gradient table with the occlusion-aware SSIM + L1 photometric term (the *_grad_ssim entries:
criterions/OSSIML1Criterion.lua:165-302 in train.lua:428-468) costs on the GPU (GPU box only): the new stage against the sum of two
stages of the same run -- table_loss_ssim, which forms the same window sums on the same planes, and table_loss_grad (or
table_loss_grad_ft with --second-order), which writes the same gradient planes.

    python tools/loss_grad_ssim_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--second-order] [--alpha 0.85]
                                        [--models random:hard:2:1.0,random:soft:2:1.0]

Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum and maximum:
  forward_loss_grad_device       Model.forwardLossGradDevice with the first-order (or, with --second-order, the fine-tuning) options
  forward_loss_ssim_device       Model.forwardLossDevice(objective="ssim")
  forward_loss_grad_ssim_device  Model.forwardLossGradDevice with loss_grad_ssim_options and the 32-word records
  equal_host                     the gradient of the first triplet equals ops.table_loss_grad (host entry, same options, the image's own
                                 range) of forward's table; checked before anything is timed, and nothing is reported without it
  equal_records                  the records of the new call equal forwardLoss(objective="ssim")'s
  table_loss_ssim, table_loss_grad | table_loss_grad_ft, table_loss_grad_ssim
                                 the stages' time per call from option profile = 1; the last with its ratio to the sum of the two before
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


def measure(model, n, H, W, reps, second, alpha):
    import torch
    m = back2future.Model(model)
    L = m.n_outputs // (5 if m.past_flow else 4)
    res = {"levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)
    opt = back2future.loss_grad_ssim_options(smooth_second_order=second, ssim_alpha=alpha)
    base = back2future.loss_grad_ft_options(smooth_second_order=True, pme_criterion="OBCC") if second else back2future.loss_grad_options()
    base_row = "table_loss_grad_ft" if second else "table_loss_grad"
    # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
    grad, rec = m.forwardLossGrad(x, options=opt, ssim_range="image")
    table = [t[:1] for t in m.forward(x)]
    res["equal_host"] = bool(same_bits([g[:1] for g in grad], ops.table_loss_grad(table, x[:1, 3:6], options=opt, ssim_range="image")))
    if not res["equal_host"]:
        m.close()
        return res
    res["equal_records"] = bool(np.array_equal(rec, m.forwardLoss(x, objective="ssim", ssim_range="image")))
    del grad, table

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    dx = torch.from_numpy(x).cuda()
    dg = [torch.empty((n,) + s, dtype=torch.float32, device="cuda") for s in m.output_shapes(H, W)]
    dl = torch.empty((n, L, 32), dtype=torch.int64, device="cuda")
    ptrs = [g.data_ptr() for g in dg]

    def grad_call(options):
        m.forwardLossGradDevice(dx.data_ptr(), n, H, W, ptrs, d_loss=dl.data_ptr(), options=options, ssim_range="image")
        torch.cuda.synchronize()

    def loss_call():
        m.forwardLossDevice(dx.data_ptr(), n, H, W, dl.data_ptr(), objective="ssim", ssim_range="image")
        torch.cuda.synchronize()

    res["forward_loss_grad_device"] = stats(host_ms(lambda: grad_call(base), reps))
    res["forward_loss_ssim_device"] = stats(host_ms(loss_call, reps))
    res["forward_loss_grad_ssim_device"] = stats(host_ms(lambda: grad_call(opt), reps))
    m.set_option("profile", 1)
    grad_call(base)
    loss_call()
    grad_call(opt)
    m.profile_reset()
    for _ in range(reps):
        grad_call(base)
        loss_call()
        grad_call(opt)
    rows = m.profile_read()
    m.set_option("profile", 0)

    def row(name):      # (table_loss_ssim runs in loss_call and in grad_call(opt): twice per repetition; the gradient stages once each)
        ms, calls = rows[name]
        return {"ms_per_call": round(ms / max(calls, 1), 4), "calls": calls}

    res["table_loss_ssim"] = row("table_loss_ssim")
    res[base_row] = row(base_row)
    res["table_loss_grad_ssim"] = row("table_loss_grad_ssim")
    yard = res["table_loss_ssim"]["ms_per_call"] + res[base_row]["ms_per_call"]
    res["table_loss_grad_ssim"]["ratio_to_ssim_plus_grad"] = round(res["table_loss_grad_ssim"]["ms_per_call"] / yard, 3)
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--second-order", action="store_true")
    ap.add_argument("--alpha", type=float, default=0.85)
    ap.add_argument("--models", default="random:hard:2:1.0,random:soft:2:1.0")
    a = ap.parse_args()
    res = {"metric": "table loss grad ssim", "n": a.n, "H": a.height, "W": a.width, "second_order": bool(a.second_order), "alpha": a.alpha}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps, a.second_order, a.alpha)
        if not res[model].get("equal_host"):
            sys.exit("%s: the gradient of the first triplet differs from the host entry's; nothing reported" % model)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
