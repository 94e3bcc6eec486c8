"""What the supervised objective (-optimize epe; train.lua:296-334 with criterions/L2Criterion.lua) costs on the GPU (GPU box only):
the route a user had before -- Model.forward, which downloads the table, and the criterion in numpy -- against
Model.forwardLossGrad(objective="epe"), and the new stage against its byte count.

    python tools/loss_epe_rate.py [--n 4] [--height 1024] [--width 1920] [--reps 5] [--models random:hard:2:1.0,random:soft:2:1.0]

Prints ONE JSON line; per model, every timing row is the median of `reps` calls with its minimum and maximum:
  forward_numpy             Model.forward(x) and the records of the flow term of every level in numpy (fp64, the library's definition)
  forward_loss_grad         Model.forwardLossGrad(x, objective="epe", ...): records and gradient table come down, the table does not
  forward_loss_grad_device  Model.forwardLossGradDevice(objective="epe") with the records: everything stays in device tensors
  equal_words               the records of forwardLossGrad equal the numpy version's word for word (words 0 .. 3; checked before
                            anything is timed, and nothing is reported without it)
  equal_host                records and gradient of the first triplet equal ops.table_loss_epe (host entry) of forward's table
  table_loss_epe            the stage's time per call from option profile = 1 inside the device call (the memsets of the records and of
                            the planes no term reaches, and the L launches of table_loss_epe_kernel), the bytes it has to move -- per
                            pixel of every level 26 read (f, o, gt_flow, valid, gt_occ) and 16 written by the kernel, and the
                            (6 | 8) floats of the warped images and the past flow that the memsets write --, and what that is in
                            bytes/s against the 6.29 TB/s a float4 copy reaches on this chip
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


def numpy_records(table, per, gt, valid, flow_scale):
    """words 0 .. 3 of the records (include/b2f.h, B2F_LOSS_EPE_*): the flow term of every level, in fp64"""
    n, _, H, W = table[0].shape
    L = len(table) // per
    rec = np.zeros((n, L, back2future.LOSS_EPE_WORDS), np.uint64)
    for j in range(L):
        s = 1 << j
        f = table[j * per].astype(np.float64)
        with np.errstate(all="ignore"):
            g = gt[:, :, ::s, ::s].astype(np.float64) / flow_scale
            d0, d1 = f[:, 0] - g[:, 0], f[:, 1] - g[:, 1]
            e = np.sqrt(d0 * d0 + d1 * d1)
        m = valid[:, ::s, ::s] != 0
        fin = np.isfinite(e)
        q = (np.minimum(np.where(fin, e, 0.0), 65536.0) * 1048576.0 + 0.5).astype(np.uint64)
        rec[:, j, back2future.LOSS_EPE_PIXELS] = (H >> j) * (W >> j)
        rec[:, j, back2future.LOSS_EPE_VALID] = (m & fin).reshape(n, -1).sum(1)
        rec[:, j, back2future.LOSS_EPE_Q20] = np.where(m & fin, q, np.uint64(0)).reshape(n, -1).sum(1, dtype=np.uint64)
        rec[:, j, back2future.LOSS_EPE_FLOW_NONFINITE] = (m & ~fin).reshape(n, -1).sum(1)
    return rec


def measure(model, n, H, W, reps):
    import torch
    m = back2future.Model(model)
    per = 5 if m.past_flow else 4
    L = m.n_outputs // per
    res = {"levels": L}
    r = np.random.default_rng(2)
    x = back2future.normalize(r.random((n * 9, H, W), dtype=np.float32)).reshape(n, 9, H, W)
    gt = (r.standard_normal((n, 2, H, W)) * 3.0).astype(np.float32)
    valid = (r.random((n, H, W)) < 0.8).astype(np.uint8)
    occ = r.integers(0, 4, (n, H, W), dtype=np.uint8)
    opt = back2future.loss_epe_options(weights={"occ": 1.0}, size_average=True)
    kw = dict(objective="epe", gt_flow=gt, valid=valid, gt_occ=occ, options=opt)
    grad, rec = m.forwardLossGrad(x, **kw)
    table = m.forward(x)
    res["equal_words"] = bool(np.array_equal(rec[:, :, :4], numpy_records(table, per, gt, valid, 20.0)[:, :, :4]))
    # the first triplet of the table of the same request (the kernels a forward pass takes follow the request's n)
    hrec, hgrad = ops.table_loss_epe([t[:1] for t in table], gt[:1], valid[:1], occ[:1], options=opt, count="image", want_grad=True)
    g1, r1 = m.forwardLossGrad(x, count="image", **kw)
    res["equal_host"] = bool(same_bits([g[:1] for g in g1], hgrad) and np.array_equal(r1[:1], hrec))
    if not (res["equal_words"] and res["equal_host"]):
        m.close()
        return res
    del grad, table, g1

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": round(med, 3), "triplets_per_s": round(n * 1e3 / med, 1), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    dx, dgt, dv, do = [torch.from_numpy(a).cuda() for a in (x, gt, valid, occ)]
    dg = [torch.empty((n,) + s, dtype=torch.float32, device="cuda") for s in m.output_shapes(H, W)]
    dl = torch.empty((n, L, back2future.LOSS_EPE_WORDS), dtype=torch.int64, device="cuda")
    ptrs = [g.data_ptr() for g in dg]

    def on_device():
        m.forwardLossGradDevice(dx.data_ptr(), n, H, W, ptrs, d_loss=dl.data_ptr(), objective="epe", gt_flow=dgt.data_ptr(), valid=dv.data_ptr(),
                                gt_occ=do.data_ptr(), options=opt)
        torch.cuda.synchronize()

    res["forward_numpy"] = stats(host_ms(lambda: numpy_records(m.forward(x), per, gt, valid, 20.0), reps))
    res["forward_loss_grad"] = stats(host_ms(lambda: m.forwardLossGrad(x, **kw), reps))
    res["forward_loss_grad_device"] = stats(host_ms(on_device, reps))
    level_px = [(H >> j) * (W >> j) for j in range(L)]
    kernel_bytes = n * (26 + 16) * sum(level_px)
    memset_bytes = n * 4 * (per * 2 + 2 - 4) * sum(level_px)   # iw1 + iw3 (6 floats) and, on a Soft table, the past flow (2)
    counting = n * 2 * sum(level_px)                           # the pre-pass of size_average: two bytes per source pixel of a level
    m.set_option("profile", 1)
    on_device()
    m.profile_reset()
    for _ in range(reps):
        on_device()
    ms, launches = m.profile_read()["table_loss_epe"]
    m.set_option("profile", 0)
    per_call = ms / max(launches, 1)
    b = kernel_bytes + memset_bytes + counting
    res["table_loss_epe"] = {"ms_per_call": round(per_call, 4), "calls": launches, "bytes": b, "kernel_bytes": kernel_bytes, "memset_bytes": memset_bytes,
                             "tb_per_s": round(b / (per_call * 1e-3) / 1e12, 3), "share_of_copy_rate": round(b / (per_call * 1e-3) / 1e12 / HBM_COPY_TB_S, 3)}
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="random:hard:2:1.0,random:soft:2:1.0")
    a = ap.parse_args()
    res = {"metric": "table loss epe", "n": a.n, "H": a.height, "W": a.width}
    for model in a.models.split(","):
        res[model] = measure(model, a.n, a.height, a.width, a.reps)
        if not (res[model].get("equal_words") and res[model].get("equal_host")):
            sys.exit("%s: the records or the gradient differ from the numpy version's or the host entry's; nothing reported" % model)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
