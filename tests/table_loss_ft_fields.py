"""Shared by tests/test_table_loss_ft_cpu.py and tests/test_gpu_table_loss_ft.py: `want_ft`, the plain numpy restatement of words
16 .. 23 of a fine-tuning record (include/b2f.h, B2F_LOSS_FT_*) that the host entry is held against, and `lua_loss_ft`, a float64
transcription of SecondOrderSmoothnessCriterion:updateOutput and OBGCCriterion:updateOutput inside the loop of test.lua:266-297 /
train.lua:428-432.  The tables are those of tests/table_loss_fields.py."""
import numpy as np

from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL

WORDS = 24
SMOOTH2_FLOW, SMOOTH2_PAST, OGX, OGY, SMOOTH2_NONFINITE, GRAD_NONFINITE = 16, 17, 18, 20, 22, 23
F32 = np.float32
# README.md:85-102 by the model names of init; what an option set does not name keeps opts.lua:61-73
OBJECTIVES = {
    "Ours-Hard": dict(past=False, second=False, criterion="OBCC", beta=1.0, gamma=1.0, weights={"pme": 1.0, "smooth_flow": 2.0}),
    "Ours-Soft-ft-KITTI": dict(past=True, second=True, criterion="OBGCC", beta=1.0, gamma=1.0,
                               weights={"pme": 2.0, "smooth_flow": 0.1, "const_vel": 0.0001}),
    "Ours-Soft-ft-Sintel": dict(past=True, second=True, criterion="OBGCC", beta=0.0, gamma=0.0,
                                weights={"pme": 4.0, "smooth_flow": 0.1, "const_vel": 0.0001}),
}


def _second(a):
    """second differences of n x C x h x w in float64, (2 a(x) - a(x-1)) - a(x+1): (gx, gy), zero on the first and last column / row"""
    a = a.astype(np.float64)
    gx, gy = np.zeros_like(a), np.zeros_like(a)
    with np.errstate(all="ignore"):
        gx[..., :, 1:-1] = (2.0 * a[..., :, 1:-1] - a[..., :, :-2]) - a[..., :, 2:]
        gy[..., 1:-1, :] = (2.0 * a[..., 1:-1, :] - a[..., :-2, :]) - a[..., 2:, :]
    return gx, gy


def _mean_abs(d):
    """the channel mean of |d|, n x 3 x h x w -> n x h x w, added left to right"""
    return ((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])) / 3.0


def second_order_weights(R):
    """(wx, wy) n x h x w of include/b2f.h: the exponent takes |R(x) - R(x-1)| on every column but the first and |R(x) - R(x+1)| on the
    interior columns; rows alike"""
    R = R.astype(np.float64)
    n, _, h, w = R.shape
    igx, igy = np.zeros((n, h, w)), np.zeros((n, h, w))
    with np.errstate(all="ignore"):
        igx[:, :, 1:] = _mean_abs(R[:, :, :, 1:] - R[:, :, :, :-1])
        igx[:, :, 1:-1] = igx[:, :, 1:-1] + _mean_abs(R[:, :, :, 1:-1] - R[:, :, :, 2:])
        igy[:, 1:, :] = _mean_abs(R[:, :, 1:, :] - R[:, :, :-1, :])
        igy[:, 1:-1, :] = igy[:, 1:-1, :] + _mean_abs(R[:, :, 1:-1, :] - R[:, :, 2:, :])
        return TL.E(-20.0 * igx), TL.E(-20.0 * igy)


def want_ft(table, ref, past, flow_scale=TL.SCALE):
    """uint64 (n, L, 8): words 16 .. 23 by the definition of include/b2f.h, one expression per word"""
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    pyr = TL.ref_pyramid(ref, L)
    rec = np.zeros((n, L, WORDS - 16), np.uint64)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    for j in range(L):
        t = table[j * per:(j + 1) * per]
        f, p, o, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
        R = pyr[j]
        h, w = R.shape[2:]
        with np.errstate(all="ignore"):
            wx, wy = second_order_weights(R)

            def smooth2(a):
                """(the q30 sum of the four products over the pixels where none is NaN, those other pixels)"""
                gx, gy = _second(a)
                prods = [P1(gx[:, 0]) * wx, P1(gy[:, 0]) * wy, P1(gx[:, 1]) * wx, P1(gy[:, 1]) * wy]
                nan = np.isnan(prods[0]) | np.isnan(prods[1]) | np.isnan(prods[2]) | np.isnan(prods[3])
                return sum(TL._q30_sum(np.where(nan, 0.0, t), ~nan) for t in prods), nan

            rec[:, j, SMOOTH2_FLOW - 16], bad = smooth2(f)
            if past:
                rec[:, j, SMOOTH2_PAST - 16], bad_p = smooth2(p)
                bad = bad | bad_p
        rec[:, j, SMOOTH2_NONFINITE - 16] = bad.reshape(n, -1).sum(axis=1)
        kd = float(F32(flow_scale / 2.0 ** j))
        rdx, rdy = TL._diffs(R)
        for d in range(2):
            fl = p if (d == 0 and past) else f
            _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
            with np.errstate(all="ignore"):
                delta = iw[d].astype(np.float64) - R.astype(np.float64)
                s = np.sqrt(delta * delta + 1e-6)
                e = (s[:, 0] + s[:, 1]) + s[:, 2]
                wt = o[:, 1 - d].astype(np.float64)
                we = wt * e
                counted = inside & ~(nan | np.isnan(e) | np.isnan(we) | np.isnan(wt))      # the pixel-directions of PHOTO_INSIDE
                idx, idy = TL._diffs(iw[d])
                ex, ey = wt[:, None] * P1(idx - rdx), wt[:, None] * P1(idy - rdy)      # n x 3 x h x w: one product per channel
            nonf = counted & (np.isnan(ex).any(axis=1) | np.isnan(ey).any(axis=1))
            good = counted & ~nonf
            rec[:, j, OGX - 16 + d] = sum(TL._q30_sum(np.where(good, ex[:, c], 0.0), good) for c in range(3))
            rec[:, j, OGY - 16 + d] = sum(TL._q30_sum(np.where(good, ey[:, c], 0.0), good) for c in range(3))
            rec[:, j, GRAD_NONFINITE - 16] += nonf.reshape(n, -1).sum(axis=1).astype(np.uint64)
    return rec


def lua_loss_ft(table, ref, past, flow_scale=TL.SCALE, like="test", size_average=False, second=True, criterion="OBGCC", beta=1.0, gamma=1.0,
                weights=None):
    """float64 array (n,): table_loss_fields.lua_loss with fs_criterion = nn.SecondOrderSmoothnessCriterion (second; model.lua:201-202,
    L1 penalty) and pme_criterion = nn.OBGCCriterion (criterion == "OBGCC"; model.lua:166-171,189-190), both updateOutput line by line
    in float64 with torch's 1-based slices turned 0-based.  Levels need h >= 3 and w >= 3, as in the reference."""
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    n_flow = 2 if past else 1
    eps = 0.001 * 0.001
    l1 = lambda x: np.power(x * x + eps, 0.5)
    quad = lambda x: x * x
    down = TL.ref_pyramid(ref, L)
    out = np.zeros(n, np.float64)

    def smoothness(inp, target, pen):            # SmoothnessCriterion.lua:28-73
        inp, target = inp.astype(np.float64), target.astype(np.float64)
        gy, gx, igy, igx = np.zeros_like(inp), np.zeros_like(inp), np.zeros_like(target), np.zeros_like(target)
        gy[:, :, :-1, :] = inp[:, :, 1:, :] - inp[:, :, :-1, :]
        gx[:, :, :, :-1] = inp[:, :, :, 1:] - inp[:, :, :, :-1]
        igy[:, :, :-1, :] = target[:, :, 1:, :] - target[:, :, :-1, :]
        igx[:, :, :, :-1] = target[:, :, :, 1:] - target[:, :, :, :-1]
        wy = np.exp(-20.0 * np.mean(np.abs(igy), axis=1, keepdims=True))
        wx = np.exp(-20.0 * np.mean(np.abs(igx), axis=1, keepdims=True))
        buf = (pen(gx) * wx + pen(gy) * wy).sum()
        return buf / inp.size if size_average else buf

    def second_order(inp, target, pen):          # SecondOrderSmoothnessCriterion.lua:28-75
        inp, target = inp.astype(np.float64), target.astype(np.float64)
        H, W = inp.shape[2:]
        assert H >= 3 and W >= 3
        gy, gx = np.zeros_like(inp), np.zeros_like(inp)
        gy[:, :, 1:H - 1, :] = 2 * inp[:, :, 1:H - 1, :] - inp[:, :, 0:H - 2, :]          # line 45
        gy[:, :, 1:H - 1, :] -= inp[:, :, 2:H, :]
        gx[:, :, :, 1:W - 1] = 2 * inp[:, :, :, 1:W - 1] - inp[:, :, :, 0:W - 2]          # line 46
        gx[:, :, :, 1:W - 1] -= inp[:, :, :, 2:W]
        igy, igx = np.zeros((inp.shape[0], 1, H, W)), np.zeros((inp.shape[0], 1, H, W))
        igy[:, :, 1:H, :] += np.mean(np.abs(target[:, :, 1:H, :] - target[:, :, 0:H - 1, :]), axis=1, keepdims=True)       # line 55
        igx[:, :, :, 1:W] += np.mean(np.abs(target[:, :, :, 1:W] - target[:, :, :, 0:W - 1]), axis=1, keepdims=True)       # line 56
        igy[:, :, 1:H - 1, :] += np.mean(np.abs(target[:, :, 1:H - 1, :] - target[:, :, 2:H, :]), axis=1, keepdims=True)   # line 57
        igx[:, :, :, 1:W - 1] += np.mean(np.abs(target[:, :, :, 1:W - 1] - target[:, :, :, 2:W]), axis=1, keepdims=True)   # line 58
        wy, wx = np.exp(-20.0 * igy), np.exp(-20.0 * igx)
        buf = (pen(gx) * wx + pen(gy) * wy).sum()                                        # line 65-66
        return buf / inp.size if size_average else buf

    def const_vel(a, b):
        d = a.astype(np.float64) - b.astype(np.float64)
        o = np.sqrt((d * d).sum(axis=1)).sum()
        return o / a.size if size_average else o

    def photometric(sub, target, scaling):       # OBCCriterion.lua:36-119 / OBGCCriterion.lua:39-149
        warp_start = 3 if past else 2            # 0-based index of the first warped image
        occ = sub[warp_start - 1].astype(np.float64)
        target = target.astype(np.float64)
        _, _, h, w = sub[0].shape
        target_gy, target_gx = np.zeros_like(target), np.zeros_like(target)
        target_gy[:, :, 0:h - 1, :] = target[:, :, 1:h, :] - target[:, :, 0:h - 1, :]    # line 67
        target_gx[:, :, :, 0:w - 1] = target[:, :, :, 1:w] - target[:, :, :, 0:w - 1]    # line 68
        img_gy, img_gx = np.zeros_like(target), np.zeros_like(target)
        cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
        cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
        acc = np.zeros((1, h, w), np.float64)
        for f in (1, 2):
            img = sub[warp_start - 1 + f].astype(np.float64)
            img_gy[:, :, 0:h - 1, :] = img[:, :, 1:h, :] - img[:, :, 0:h - 1, :]          # line 91 (the last row stays 0)
            img_gx[:, :, :, 0:w - 1] = img[:, :, :, 1:w] - img[:, :, :, 0:w - 1]          # line 92
            tmp = l1(img - target).sum(axis=1)                                           # line 97: no alpha
            if criterion == "OBGCC":
                tmp = tmp + l1(img_gx - target_gx).sum(axis=1) * beta                    # line 101
                tmp = tmp + l1(img_gy - target_gy).sum(axis=1) * gamma                   # line 105
            if f <= 1.0:
                fl = sub[1] if past else sub[0]
                tx = cx + (F32(f - 1 - 1) * fl[:, 0]) * F32(scaling)
                ty = cy + (F32(f - 1 - 1) * fl[:, 1]) * F32(scaling)
                tmp = tmp * occ[:, 1]
            else:
                tx = cx + (F32(f - 1) * sub[0][:, 0]) * F32(scaling)
                ty = cy + (F32(f - 1) * sub[0][:, 1]) * F32(scaling)
                tmp = tmp * occ[:, 0]
            mask = ((tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)).astype(np.float64)
            acc += tmp * mask + (1.0 - mask) * 1.0
        o = acc.sum() / (3 * 2)
        return o * (3.0 / (3.0 * h * w)) if size_average else o

    def prior(occ):
        occ = occ.astype(np.float64)
        o = (1.0 - occ[:, 0] * occ[:, 1]).sum()
        return o * (2.0 / occ.size) if size_average else o

    fs = second_order if second else smoothness
    for b in range(n):
        err = 0.0
        for l in range(L):
            sub = [t[b:b + 1] for t in table[l * per:(l + 1) * per]]
            target = down[l][b:b + 1]
            lw = TL.LEVEL_WEIGHTS[l]
            for i in range(n_flow):              # test.lua:275-277 passes sub_outs[1] every time, train.lua:428-432 sub_outs[i]
                err += lw * wt["smooth_flow"] * fs(sub[0 if like == "test" else i], target, l1)
            if past:
                err += lw * wt["const_vel"] * const_vel(sub[0], sub[1])
            err += lw * wt["pme"] * photometric(sub, target, flow_scale / 2.0 ** l)
            err += lw * wt["smooth_occ"] * smoothness(sub[per - 3], target, quad)
            err += lw * wt["prior_occ"] * prior(sub[per - 3])
        out[b] = err
    return out


def bound_ft(H, W, L, past, second=True, criterion="OBGCC", beta=1.0, gamma=1.0, size_average=False, weights=None, lua=0.0):
    """table_loss_fields.bound for the fine-tuning terms: each pixel term rounds by at most 2^-31 in the record, so the difference is
    at most the sum over levels and terms of level_weight * weight * (pixel terms) * 2^-31 (times the term's norm with
    size_average), plus 1e-12 * |lua| for the float64 sums of the transcription.  The first-order flow smoothness has one rounded
    term per pixel and flow taken, the second-order one four (channel x axis); OBGCC has per pixel and direction one brightness
    term and three gradient terms (the channels) per axis, weighted 1, beta and gamma."""
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    n_flow = 2 if past else 1
    per_dir = 1.0 + (3.0 * (abs(beta) + abs(gamma)) if criterion == "OBGCC" else 0.0)
    per_flow = 4.0 if second else 1.0
    total = 0.0
    for j in range(L):
        hw = float((H >> j) * (W >> j))
        half, full = (1.0 / (2.0 * hw), 1.0 / hw) if size_average else (1.0, 1.0)
        t = wt["smooth_flow"] * n_flow * per_flow * hw * half
        t += (wt["const_vel"] * hw * half) if past else 0.0
        t += wt["pme"] * (per_dir * 2.0 * hw / 6.0) * full
        t += wt["smooth_occ"] * hw * half + wt["prior_occ"] * hw * full
        total += TL.LEVEL_WEIGHTS[j] * t * 2.0 ** -31
    return total + 1e-12 * abs(lua)
