"""Shared by tests/test_table_loss_epe_cpu.py and tests/test_gpu_table_loss_epe.py: the ground truth the supervised objective
(-optimize epe; train.lua:296-334 with criterions/L2Criterion.lua:27-71) is tested on, `want`, the plain numpy restatement of
include/b2f.h's definition of its records and gradient table that the host entry is held against bit for bit, and `lua_epe`, a float64
transcription of L2Criterion.lua and of the loop of train.lua:296-334 written from the Lua text."""
import numpy as np

from tests import table_loss_fields as TL

F32 = np.float32
WORDS = 8
PIXELS, VALID, EPE_Q20, FLOW_NONFINITE, LABELLED, OCC_Q20, OCC_NONFINITE = 0, 1, 2, 3, 4, 5, 6
BATCH, IMAGE, GIVEN = 0, 1, 2
LEVEL_WEIGHTS = (0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28)   # train.lua:56-58
EPS = 1e-12                                                   # L2Criterion.lua:20
# 1 x 1 .. 5 x 7: one pixel, one row, one column, less than a group, a group and a tail; 37 x 53: odd, several groups per row, rows that
# are not 16-byte aligned; (16,16,5): the coarsest levels are 2 x 2 and 1 x 1; (48,80,5): widths 80 .. 5, strides 1 .. 16
SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 3, 1), (3, 3, 1), (4, 4, 1), (5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)]
VALID_KINDS = (None, "zero", "one", "random")


def opts(epe=1.0, occ=0.0, size_average=False, level_weights=LEVEL_WEIGHTS):
    return {"epe": float(epe), "occ": float(occ), "size_average": bool(size_average), "level_weights": tuple(float(v) for v in level_weights)}


def struct(o):
    from back2future_amd import back2future
    return back2future.loss_epe_options(weights={"epe": o["epe"], "occ": o["occ"], "level_weights": o["level_weights"]}, size_average=o["size_average"])


def ground_truth(table, past, flow_scale, rescale, valid_kind="random", seed=0, hit=True, empty_level=None):
    """(table', gt_flow, valid, gt_occ) for a table of TL.tables: gt_flow n x 2 x H x W float32 in pixels, N(0, 12); valid None, all zero,
    one pixel (the last one of image 0) or random, with 1e9 (Sintel's marker) and NaN under valid == 0; gt_occ bytes 0 / 1 / 2 and the
    unlabelled 3, 7 and 255.  hit: source pixel (0, 0) carries 40 px and the estimate of every level is set to the same flow there
    (40 / flow_scale / 2^j is a float), so that e is exactly 0, with valid set; table' is the table with those elements replaced.
    empty_level=j: every source pixel of level j is invalid except those that only finer levels read (needs j >= 1)."""
    per = 5 if past else 4
    n, _, H, W = table[0].shape
    r = np.random.default_rng(seed * 7919 + H * 131 + W)
    gt = (r.standard_normal((n, 2, H, W)) * 12.0).astype(F32)
    occ = r.choice(np.array([0, 1, 2, 3, 7, 255], np.uint8), size=(n, H, W))
    if valid_kind is None:
        valid = None
    elif valid_kind == "zero":
        valid = np.zeros((n, H, W), np.uint8)
    elif valid_kind == "one":
        valid = np.zeros((n, H, W), np.uint8)
        valid[0, H - 1, W - 1] = 1
    else:
        valid = (r.random((n, H, W)) < 0.7).astype(np.uint8) * r.choice(np.array([1, 2, 255], np.uint8), size=(n, H, W))
    if empty_level is not None:
        s = 1 << empty_level
        valid = np.ones((n, H, W), np.uint8) if valid is None else valid
        valid[:, ::s, ::s] = 0
    table = [t.copy() for t in table]
    if hit and valid_kind != "zero" and empty_level is None:
        gt[:, :, 0, 0] = F32(40.0)
        if valid is not None:
            valid[:, 0, 0] = 1
        for j in range(len(table) // per):
            table[j * per][:, :, 0, 0] = F32(40.0 / flow_scale / ((1 << j) if rescale else 1))
    if valid is not None:
        bad = valid == 0
        marker = np.where(r.random((n, H, W)) < 0.5, F32(1e9), F32(np.nan)).astype(F32)
        for c in range(2):
            gt[:, c][bad] = marker[bad]
    return table, gt, valid, np.ascontiguousarray(occ)


def counts_of(valid, gt_occ, n, H, W, L):
    """n x L x 2: the valid and the labelled source pixels of every image and level"""
    c = np.zeros((n, L, 2), np.float64)
    for j in range(L):
        s = 1 << j
        v = np.ones((n, H >> j, W >> j), bool) if valid is None else valid[:, ::s, ::s][:, :H >> j, :W >> j] != 0
        c[:, j, 0] = v.reshape(n, -1).sum(1)
        if gt_occ is not None:
            c[:, j, 1] = (gt_occ[:, ::s, ::s][:, :H >> j, :W >> j] < 3).reshape(n, -1).sum(1)
    return c


def level_counts(o, valid, gt_occ, n, H, W, L, count_mode, counts):
    """N_j, N'_j as n x L x 2 for the mode"""
    own = counts_of(valid, gt_occ if o["occ"] > 0 else None, n, H, W, L)
    if count_mode == GIVEN:
        return np.broadcast_to(np.asarray(counts, np.float64)[None], (n, L, 2)).copy()
    if count_mode == BATCH:
        return np.broadcast_to(own.sum(0, keepdims=True), (n, L, 2)).copy()
    return own


def _term(d0, d1, k, mask):
    """L2Criterion on masked pixels: (counted, nonfinite, q20, g0, g1) as arrays; fp64, one numpy operation per rounding"""
    with np.errstate(all="ignore"):
        e = np.sqrt(d0 * d0 + d1 * d1)
        fin = np.isfinite(e)
        q = (np.minimum(np.where(fin, e, 0.0), 65536.0) * 1048576.0 + 0.5).astype(np.uint64)
        den = e + EPS
        g = [np.where(mask & (k != 0.0), (k * d) / den, 0.0) for d in (d0, d1)]
    return mask & fin, mask & ~fin, np.where(mask & fin, q, np.uint64(0)), g[0], g[1]


def want(table, past, gt_flow, valid, gt_occ, flow_scale, rescale, o, count_mode=BATCH, counts=None):
    """(records uint64 n x L x 8, gradient table): include/b2f.h's definition of the *_epe entries in numpy"""
    per = 5 if past else 4
    L = len(table) // per
    n, _, H, W = table[0].shape
    N = level_counts(o, valid, gt_occ, n, H, W, L, count_mode, counts)
    rec = np.zeros((n, L, WORDS), np.uint64)
    grad = [np.zeros(t.shape, F32) for t in table]
    for j in range(L):
        h, w, s = H >> j, W >> j, 1 << j
        sub = lambda a: a[..., ::s, ::s][..., :h, :w]
        lw = 1.0 if o["size_average"] else o["level_weights"][j]
        f, oc = table[j * per].astype(np.float64), table[j * per + per - 3].astype(np.float64)
        with np.errstate(all="ignore"):
            g = (sub(gt_flow).astype(np.float64) / flow_scale) / (float(s) if rescale else 1.0)
        for b in range(n):
            kf, ko = o["epe"] * lw, o["occ"] * lw
            if o["size_average"]:
                kf = kf / N[b, j, 0] if N[b, j, 0] > 0 else 0.0
                ko = ko / N[b, j, 1] if N[b, j, 1] > 0 else 0.0
            m = np.ones((h, w), bool) if valid is None else sub(valid[b]) != 0
            with np.errstate(all="ignore"):
                cnt, nonf, q, g0, g1 = _term(f[b, 0] - g[b, 0], f[b, 1] - g[b, 1], kf, m)
            rec[b, j, PIXELS] = h * w
            rec[b, j, VALID], rec[b, j, FLOW_NONFINITE], rec[b, j, EPE_Q20] = cnt.sum(), nonf.sum(), q.sum(dtype=np.uint64)
            grad[j * per][b, 0], grad[j * per][b, 1] = g0.astype(F32), g1.astype(F32)
            if o["occ"] > 0:
                lab = sub(gt_occ[b])
                t0 = np.where(lab == 0, 1.0, np.where(lab == 1, 0.5, 0.0))
                t1 = np.where(lab == 2, 1.0, np.where(lab == 1, 0.5, 0.0))
                with np.errstate(all="ignore"):
                    cnt, nonf, q, g0, g1 = _term(oc[b, 0] - t0, oc[b, 1] - t1, ko, lab < 3)
                rec[b, j, LABELLED], rec[b, j, OCC_NONFINITE], rec[b, j, OCC_Q20] = cnt.sum(), nonf.sum(), q.sum(dtype=np.uint64)
                grad[j * per + per - 3][b, 0], grad[j * per + per - 3][b, 1] = g0.astype(F32), g1.astype(F32)
    return rec, grad


# ---- the reference, from the Lua text ----

def l2_forward(inp, target, mask, size_average):
    """L2Criterion:updateOutput (lines 27-45): input / target b x 2 x h x w, mask b x 1 x h x w"""
    npixels = mask.sum()                                              # line 34
    buffer = (inp + -1 * target) ** 2                                 # line 36
    epe_map = np.sqrt(buffer.sum(1, keepdims=True)) * mask            # line 37
    output = epe_map.sum()                                            # line 38
    return output / npixels if size_average else output              # lines 40-42


def l2_backward(inp, target, mask, size_average):
    """L2Criterion:updateGradInput (lines 47-71)"""
    npixels = mask.sum()                                              # line 56
    buffer = (inp + -1 * target) ** 2                                 # line 58
    loss = np.sqrt(buffer.sum(1, keepdims=True) * mask) + EPS         # line 59
    loss = np.repeat(loss, inp.shape[1], 1)                           # line 60
    rep_mask = np.repeat(mask, inp.shape[1], 1)                       # line 62
    grad = (inp + -1 * target) / loss * rep_mask                      # line 64
    return grad / npixels if size_average else grad                   # lines 66-68


def lua_epe(table, past, gt_flow, valid, gt_occ, flow_scale, rescale, o):
    """train.lua:296-334 in float64 over the whole batch (the reference's count is the batch's): (err, flow part per level, occlusion part
    per level, gradient table, epe of train.lua:340-344).  The labels are the ground truth over flownet_factor, as train.lua:340 undoes;
    the occlusion target is the one lines 324-325 intend, the criterion's mask the labelled pixels.  Ground truth and estimates must be
    finite: the Lua multiplies by the mask, it does not select."""
    per = 5 if past else 4
    L = len(table) // per
    n, _, H, W = table[0].shape
    down_nn = lambda a: a[:, :, ::2, ::2]                             # nn.SpatialAveragePooling(1,1,2,2), line 282
    level_weights = [1.0] * 7 if o["size_average"] else list(o["level_weights"])   # lines 56-64
    flow = gt_flow.astype(np.float64) / flow_scale
    mask = (np.ones((n, 1, H, W)) if valid is None else (valid != 0).astype(np.float64).reshape(n, 1, H, W))
    lab = None if gt_occ is None else gt_occ.reshape(n, 1, H, W)
    err, parts_f, parts_o = 0.0, [], []
    grad = [np.zeros(t.shape, np.float64) for t in table]             # lines 290-292
    for l in range(L):
        if l > 0:                                                     # lines 297-306
            flow, mask = down_nn(flow), down_nn(mask)
            if rescale:
                flow = flow / 2
            if lab is not None:
                lab = down_nn(lab)
        out_f = table[l * per].astype(np.float64)
        err_f = o["epe"] * l2_forward(out_f, flow, mask, o["size_average"])                          # line 312
        err += err_f * level_weights[l]                                                               # line 313
        grad[l * per] += l2_backward(out_f, flow, mask, o["size_average"]) * (o["epe"] * level_weights[l])   # line 314
        parts_f.append(err_f * level_weights[l])
        tmp = 0.0
        if o["occ"] > 0:
            t = np.concatenate([(lab == 0) + 0.5 * (lab == 1), (lab == 2) + 0.5 * (lab == 1)], 1).astype(np.float64)   # lines 324-325
            m = (lab < 3).astype(np.float64)
            out_o = table[l * per + per - 3].astype(np.float64)
            tmp = o["occ"] * level_weights[l] * l2_forward(out_o, t, m, o["size_average"])            # line 328
            err += tmp                                                                                # line 329
            grad[l * per + per - 3] += l2_backward(out_o, t, m, o["size_average"]) * (o["occ"] * level_weights[l])   # line 331
        parts_o.append(tmp)
    mask0 = np.ones((n, 1, H, W)) if valid is None else (valid != 0).astype(np.float64).reshape(n, 1, H, W)
    epe_b = l2_forward(table[0].astype(np.float64) * flow_scale, gt_flow.astype(np.float64), mask0, False) / mask0.sum()   # lines 340-343
    return err, np.array(parts_f), np.array(parts_o), grad, epe_b


def finite_truth(table, past, flow_scale, seed=0):
    """ground truth for the comparisons with the Lua: finite everywhere, valid random (1e9 / NaN under valid == 0 have no meaning in a
    criterion that multiplies by its mask), labels 0 / 1 / 2 / 3"""
    n, _, H, W = table[0].shape
    r = np.random.default_rng(seed + 17)
    gt = (r.standard_normal((n, 2, H, W)) * 12.0).astype(F32)
    valid = (r.random((n, H, W)) < 0.7).astype(np.uint8)
    occ = r.choice(np.array([0, 1, 2, 3], np.uint8), size=(n, H, W))
    return gt, valid, np.ascontiguousarray(occ)


def tables(H, W, L, past, n=2, tame=False, seed=0):
    return TL.tables(H, W, L, past, n=n, seed=seed, tame=tame)[0]
