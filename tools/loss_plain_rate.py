"""What the photometric terms without occlusion masking (the *_plain and *_grad_plain entries: criterions/MBCCriterion.lua and
criterions/MSSIML1Criterion.lua in test.lua:266-297 / train.lua:428-468) cost on the GPU (GPU box only), against the route a user had
before -- Model.forward, the table down the link, the criterion in numpy -- and, stage by stage, against the occlusion-aware siblings of
the same run: table_loss_plain against table_loss_ssim (the same window sums on the same planes, plus the raw differences) and
table_loss_grad_plain against table_loss_grad_ssim.

    python tools/loss_plain_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--numpy-reps 5]
                                    [--models random:hard:2:1.0,random:soft:2:1.0]

Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum and maximum:
  equal_host                      the records and the SSIML1 and BCC gradients of the first triplet equal the host entries' (the image's own
                                  range) on forward's table; checked before anything is timed, and nothing is reported without it
  equal_records                   the records beside the gradient equal forwardLoss(objective="plain")'s
  forward_numpy                   the old route: Model.forward (the table comes down) and MSSIML1Criterion's value in numpy float64
  forward_loss_plain              Model.forwardLoss(objective="plain") and loss_summary(pme_criterion="SSIML1"): 320 bytes per level come down
  numpy_against_records           the largest relative difference of the two routes' photometric value per triplet
  forward_loss_ssim_device, forward_loss_plain_device, forward_loss_grad_ssim_device, forward_loss_grad_plain_device (SSIML1),
  forward_loss_grad_plain_bcc_device
  stages                          per stage, from option profile = 1 around each single call: median, minimum and maximum of the reps;
                                  over_yardstick: the new stage's median minus its yardstick's median, and allowed: the yardstick's own
                                  max - min
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


def numpy_mssiml1(table, ref, past, flow_scale=20.0, alpha=0.85):
    """MSSIML1Criterion:updateOutput (lines 45-153) per triplet and level in numpy float64, each triplet a batch of one: the value a user
    computed from the downloaded table.  -> (n, L) array"""
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    e = np.exp(-8.0 / 9.0)
    ge, gc = e / (1.0 + 2.0 * e), 1.0 / (1.0 + 2.0 * e)

    def G(a):
        p = np.pad(a, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge")
        col = ge * p[:, :, :-2, :] + gc * p[:, :, 1:-1, :] + ge * p[:, :, 2:, :]
        return ge * col[:, :, :, :-2] + gc * col[:, :, :, 1:-1] + ge * col[:, :, :, 2:]

    out = np.zeros((n, L))
    R = np.asarray(ref, np.float32)
    for j in range(L):
        if j:
            R = ((R[:, :, 0::2, 0::2] + R[:, :, 0::2, 1::2]) + R[:, :, 1::2, 0::2] + R[:, :, 1::2, 1::2]) / np.float32(4)
        t = table[j * per:(j + 1) * per]
        h, w = R.shape[2:]
        k = np.float32(flow_scale / 2.0 ** j)
        cx, cy = np.arange(w, dtype=np.float32)[None, None, :], np.arange(h, dtype=np.float32)[None, :, None]
        for b in range(n):
            planes = [R[b]] + [x[b] for x in t[1:]]
            mn, mx = float(min(p.min() for p in planes)), float(max(p.max() for p in planes))
            y = (R[b:b + 1].astype(np.float64) - mn) / (mx - mn)
            mu_y = G(y)
            s_y = G(y * y) - mu_y * mu_y
            acc = 0.0
            for d in range(2):
                fl = t[1] if (d == 0 and past) else t[0]
                tx, ty = cx + fl[b:b + 1, 0] * (-k if d == 0 else k), cy + fl[b:b + 1, 1] * (-k if d == 0 else k)
                mask = (tx >= 0) & (ty >= 0) & (tx <= w - 1) & (ty <= h - 1)
                x = (t[per - 2 + d][b:b + 1].astype(np.float64) - mn) / (mx - mn)
                mu_x = G(x)
                s_x, s_xy = G(x * x) - mu_x * mu_x, G(x * y) - mu_x * mu_y
                l = (2 * mu_x * mu_y + 1e-4) / (mu_x * mu_x + mu_y * mu_y + 1e-4)
                cs = (2 * s_xy + 9e-4) / (s_x + s_y + 9e-4)
                tmp = alpha * (1 - l * cs).sum(1) + (1 - alpha) * np.sqrt((x - y) ** 2 + 1e-6).sum(1)
                acc += float((tmp * mask).sum())
            out[b, j] = acc / 6.0
    return out


def measure(model, n, H, W, reps, numpy_reps):
    import torch
    m = back2future.Model(model)
    past = bool(m.past_flow)
    L = m.n_outputs // (5 if past else 4)
    res = {"levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)
    opt = back2future.loss_grad_plain_options(pme_criterion="SSIML1")
    bcc = back2future.loss_grad_plain_options(pme_criterion="BCC", no_occ=True)
    yard = back2future.loss_grad_ssim_options()
    # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
    grad, rec = m.forwardLossGrad(x, options=opt, ssim_range="image")
    gbcc = m.forwardLossGrad(x, options=bcc, ssim_range="image", want_loss=False)
    full = m.forward(x)
    table = [t[:1] for t in full]
    res["equal_host"] = bool(same_bits([g[:1] for g in grad], ops.table_loss_grad(table, x[:1, 3:6], options=opt, ssim_range="image")) and
                             same_bits([g[:1] for g in gbcc], ops.table_loss_grad(table, x[:1, 3:6], options=bcc, ssim_range="image")) and
                             np.array_equal(rec[:1], ops.table_loss(table, x[:1, 3:6], objective="plain", ssim_range="image")))
    if not res["equal_host"]:
        m.close()
        return res
    res["equal_records"] = bool(np.array_equal(rec, m.forwardLoss(x, objective="plain", ssim_range="image")))
    # the two routes give the same photometric value (size_average off; the records round each pixel term by 2^-31)
    s = back2future.loss_summary(rec, pme_criterion="SSIML1")
    want = numpy_mssiml1(full, x[:, 3:6], past)
    res["numpy_against_records"] = float(np.abs(s["pme"] - want).max() / np.abs(want).max())
    del grad, gbcc, table, full

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def old_route():
        t = m.forward(x)
        return numpy_mssiml1(t, x[:, 3:6], past)

    def new_route():
        return back2future.loss_summary(m.forwardLoss(x, objective="plain", ssim_range="image"), pme_criterion="SSIML1")

    res["forward_numpy"] = stats(host_ms(old_route, numpy_reps))
    res["forward_loss_plain"] = stats(host_ms(new_route, reps))
    dx = torch.from_numpy(x).cuda()
    dg = [torch.empty((n,) + s, dtype=torch.float32, device="cuda") for s in m.output_shapes(H, W)]
    dl = torch.empty((n, L, 40), dtype=torch.int64, device="cuda")
    ptrs = [g.data_ptr() for g in dg]

    def grad_call(options):
        m.forwardLossGradDevice(dx.data_ptr(), n, H, W, ptrs, d_loss=dl.data_ptr(), options=options, ssim_range="image")
        torch.cuda.synchronize()

    def loss_call(objective):
        m.forwardLossDevice(dx.data_ptr(), n, H, W, dl.data_ptr(), objective=objective, ssim_range="image")
        torch.cuda.synchronize()

    calls = [("forward_loss_ssim_device", lambda: loss_call("ssim")), ("forward_loss_plain_device", lambda: loss_call("plain")),
             ("forward_loss_grad_ssim_device", lambda: grad_call(yard)), ("forward_loss_grad_plain_device", lambda: grad_call(opt)),
             ("forward_loss_grad_plain_bcc_device", lambda: grad_call(bcc))]
    for name, call in calls:
        res[name] = stats(host_ms(call, reps))
    # the stages, one call at a time, so that each has its own spread
    m.set_option("profile", 1)
    per_call = {"table_loss_ssim": [], "table_loss_plain": [], "table_loss_grad_ssim": [], "table_loss_grad_plain": [], "table_loss_grad_plain_bcc": []}
    for name, call in calls:
        call()
    for _ in range(reps):
        for name, call, row, key in ((calls[0] + ("table_loss_ssim", "table_loss_ssim")), (calls[1] + ("table_loss_plain", "table_loss_plain")),
                                     (calls[2] + ("table_loss_grad_ssim", "table_loss_grad_ssim")),
                                     (calls[3] + ("table_loss_grad_plain", "table_loss_grad_plain")),
                                     (calls[4] + ("table_loss_grad_plain", "table_loss_grad_plain_bcc"))):
            m.profile_reset()
            call()
            ms, cnt = m.profile_read()[row]
            per_call[key].append(ms / max(cnt, 1))
    m.set_option("profile", 0)
    st = {}
    for key, ms in per_call.items():
        st[key] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    for new, old in (("table_loss_plain", "table_loss_ssim"), ("table_loss_grad_plain", "table_loss_grad_ssim"),
                     ("table_loss_grad_plain_bcc", "table_loss_grad_ssim")):
        st[new]["over_yardstick"] = round(st[new]["ms"] - st[old]["ms"], 4)
        st[new]["allowed"] = round(st[old]["max_ms"] - st[old]["min_ms"], 4)
    res["stages"] = st
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-reps", type=int, default=5)
    ap.add_argument("--models", default="random:hard:2:1.0,random:soft:2:1.0")
    a = ap.parse_args()
    res = {"metric": "table loss plain", "n": a.n, "H": a.height, "W": a.width}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps, a.numpy_reps)
        if not res[model].get("equal_host"):
            sys.exit("%s: the first triplet differs from the host entries'; nothing reported" % model)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
