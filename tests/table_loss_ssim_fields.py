"""Shared by tests/test_table_loss_ssim_cpu.py and tests/test_gpu_table_loss_ssim.py: `want_ssim`, the plain numpy restatement of
words 16 .. 25 of an SSIM record (include/b2f.h, B2F_LOSS_SSIM_*) that the host entry is held against, `lua_loss_ssim`, a float64
transcription of OSSIML1Criterion:updateOutput (criterions/OSSIML1Criterion.lua:47-163) inside the loop of test.lua:266-297 /
train.lua:428-432 that shares nothing with the restatement (a 2-D kernel from the Gaussian formula, torch's replicate padding and
conv2d), and `bound_ssim` / `allowance_ssim`, the bar between the two.  The tables are those of tests/table_loss_fields.py."""
import ctypes as C

import numpy as np

from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL

WORDS = 32
SSIM, L1N, SSIM_NONFINITE, RANGE_USED, RANGE_OWN = 16, 18, 20, 22, 24
BATCH, IMAGE, GIVEN = 0, 1, 2
ALPHA = {"OSSIM": 1.0, "OSSIML1": 0.85}      # model.lua:172-179
C1, C2 = 0.01 ** 2, 0.03 ** 2                # OSSIML1Criterion.lua:78-79 with L = 1
F32 = np.float32
MUTATIONS = ("zero_padding", "swapped_weights", "wrong_occlusion", "raw_l1")


def weights():
    """(ge, gc) as the library states them (b2f_loss_ssim_weights): the restatement does not restate them"""
    from back2future_amd import _lib
    out = (C.c_double * 2)()
    _lib.check(_lib.lib().b2f_loss_ssim_weights(out))
    return float(out[0]), float(out[1])


def _enc(v):
    """the order-preserving unsigned encoding of float32 values (-0 below +0)"""
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _dec_bits(e):
    e = np.uint32(e)
    return np.uint32(e & np.uint32(0x7fffffff)) if e & np.uint32(0x80000000) else np.uint32(~e)


def own_range_bits(planes):
    """(bits of the minimum, bits of the maximum) over float32 arrays, NaNs skipped, infinities kept; of no values: two NaNs"""
    v = np.concatenate([np.ascontiguousarray(p, F32).ravel() for p in planes])
    v = v[~np.isnan(v)]
    if v.size == 0:
        return _dec_bits(0xffffffff), _dec_bits(0)
    e = _enc(v)
    return _dec_bits(e.min()), _dec_bits(e.max())


def _as_float(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def _window(a, ge, gc, zero_padding=False):
    """G of n x C x h x w float64 in the fixed order of include/b2f.h: columns first, indices clamped to the plane"""
    pad = [(0, 0), (0, 0), (1, 1), (1, 1)]
    p = np.pad(a, pad, mode="constant") if zero_padding else np.pad(a, pad, mode="edge")
    with np.errstate(all="ignore"):
        col = (ge * p[:, :, :-2, :] + gc * p[:, :, 1:-1, :]) + ge * p[:, :, 2:, :]
        return (ge * col[:, :, :, :-2] + gc * col[:, :, :, 1:-1]) + ge * col[:, :, :, 2:]


def want_ssim(table, ref, past, flow_scale=TL.SCALE, mode=BATCH, ranges=None, mutation=None):
    """uint64 (n, L, 10): words 16 .. 25 by the definition of include/b2f.h, one expression per word.  mutation: one of MUTATIONS, a
    wrong reading of the definition that the tests must tell from the right one."""
    assert mutation is None or mutation in MUTATIONS
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    pyr = TL.ref_pyramid(ref, L)
    ge, gc = weights()
    if mutation == "swapped_weights":
        ge, gc = gc, ge
    rec = np.zeros((n, L, 10), np.uint64)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    for j in range(L):
        t = table[j * per:(j + 1) * per]
        f, p, o, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
        R = pyr[j]
        own = [own_range_bits([R[b], iw[0][b], iw[1][b]]) for b in range(n)]
        if mode == BATCH:
            both = own_range_bits([R, iw[0], iw[1]])
            used = [both] * n
        elif mode == IMAGE:
            used = own
        else:
            g = np.asarray(ranges, F32).reshape(L, 2)[j].view(np.uint32)
            used = [(g[0], g[1])] * n
        kd = float(F32(flow_scale / 2.0 ** j))
        for b in range(n):
            rec[b, j, RANGE_OWN - 16], rec[b, j, RANGE_OWN - 15] = own[b]
            rec[b, j, RANGE_USED - 16], rec[b, j, RANGE_USED - 15] = used[b]
            mn, mx = _as_float(used[b][0]), _as_float(used[b][1])
            ok = bool(mx > mn) and bool(np.isfinite(mn)) and bool(np.isfinite(mx))
            with np.errstate(all="ignore"):
                norm = lambda a: (a[b:b + 1].astype(np.float64) - np.float64(mn)) / (np.float64(mx) - np.float64(mn))
                y = norm(R)
                zp = mutation == "zero_padding"
                mu_y = _window(y, ge, gc, zp)
                s_y = _window(y * y, ge, gc, zp) - mu_y * mu_y
            for d in range(2):
                fl = p if (d == 0 and past) else f
                _, _, nan, inside = FW.coordinates(fl[b:b + 1], -kd if d == 0 else kd)
                with np.errstate(all="ignore"):
                    delta = iw[d][b:b + 1].astype(np.float64) - R[b:b + 1].astype(np.float64)
                    s = np.sqrt(delta * delta + 1e-6)
                    e = (s[:, 0] + s[:, 1]) + s[:, 2]
                    wt = o[b:b + 1, 1 - d].astype(np.float64)
                    we = wt * e
                    counted = inside & ~(nan | np.isnan(e) | np.isnan(we) | np.isnan(wt))      # the pixel-directions of PHOTO_INSIDE
                    if mutation == "wrong_occlusion":
                        wt = o[b:b + 1, d].astype(np.float64)
                    x = norm(iw[d])
                    mu_x = _window(x, ge, gc, zp)
                    s_x = _window(x * x, ge, gc, zp) - mu_x * mu_x
                    s_xy = _window(x * y, ge, gc, zp) - mu_x * mu_y
                    l = (2.0 * (mu_x * mu_y) + 1e-4) / ((mu_x * mu_x + mu_y * mu_y) + 1e-4)
                    cs = (2.0 * s_xy + 9e-4) / ((s_x + s_y) + 9e-4)
                    one = 1.0 - l * cs
                    S = (one[:, 0] + one[:, 1]) + one[:, 2]
                    pd = P1(delta) if mutation == "raw_l1" else P1(x - y)
                    B = (pd[:, 0] + pd[:, 1]) + pd[:, 2]
                    ws, wb = wt * S, wt * B
                if not ok:
                    rec[b, j, SSIM_NONFINITE - 16 + d] = counted.sum()
                    continue
                nonf = counted & (np.isnan(ws) | np.isnan(wb))
                good = counted & ~nonf
                rec[b, j, SSIM - 16 + d] = TL._q30_sum(np.where(good, ws, 0.0), good)[0]
                rec[b, j, L1N - 16 + d] = TL._q30_sum(np.where(good, wb, 0.0), good)[0]
                rec[b, j, SSIM_NONFINITE - 16 + d] = nonf.sum()
    return rec


def gaussian3():
    """image.gaussian{size = 3, normalize = true} as include/b2f.h restates it: sigma = 0.25 * size, the centre on the middle tap, an
    unnormalised tap at distance (dy, dx) = exp(-((dx / 0.75)^2 + (dy / 0.75)^2) / 2), the nine normalised to sum 1"""
    d = np.arange(3, dtype=np.float64) - 1.0
    k = np.exp(-((d[None, :] / 0.75) ** 2 + (d[:, None] / 0.75) ** 2) / 2.0)
    return k / k.sum()


def ossiml1(sub, target, past, scaling, alpha, mn, mx, size_average):
    """OSSIML1Criterion:updateOutput on one triplet (lines 47-163) in float64, line by line; mn, mx: the range of lines 62-67, which
    the caller takes over the batch the reference would have seen"""
    import torch
    import torch.nn.functional as F
    weight = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
    for c in range(3):
        weight[c, c] = torch.from_numpy(gaussian3())                               # lines 38-44
    conv = lambda a: F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), weight)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    warp_start = 3 if past else 2          # 0-based index of the first warped image
    _, _, h, w = sub[0].shape
    y = (T(target) - mn) / (mx - mn)                                               # line 72
    occ = T(sub[warp_start - 1])
    cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
    cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
    acc = torch.zeros(1, h, w, dtype=torch.float64)
    mu_y = conv(y)                                                                 # line 97
    sigma_y = conv(y ** 2) - mu_y ** 2                                             # line 98
    for f in (1, 2):
        img = (T(sub[warp_start - 1 + f]) - mn) / (mx - mn)                        # line 102
        buffer = img - y                                                           # line 107
        mu_x = conv(img)
        sigma_x = conv(img ** 2) - mu_x ** 2
        sigma_xy = conv(img * y) - mu_x * mu_y
        ssim_l = (2 * mu_x * mu_y + C1) / (mu_x ** 2 + mu_y ** 2 + C1)             # line 115
        ssim_cs = (2 * sigma_xy + C2) / (sigma_x + sigma_y + C2)                   # line 116
        tmp = alpha * (1 - ssim_l * ssim_cs).sum(1) + (1 - alpha) * torch.sqrt(buffer * buffer + 0.001 * 0.001).sum(1)   # line 119
        if f <= 1.0:
            fl = sub[1] if past else sub[0]
            tx = cx + (F32(f - 1 - 1) * fl[:, 0]) * F32(scaling)
            ty = cy + (F32(f - 1 - 1) * fl[:, 1]) * F32(scaling)
            tmp = tmp * occ[:, 1]
        else:
            tx = cx + (F32(f - 1) * sub[0][:, 0]) * F32(scaling)
            ty = cy + (F32(f - 1) * sub[0][:, 1]) * F32(scaling)
            tmp = tmp * occ[:, 0]
        mask = torch.from_numpy(((tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)).astype(np.float64))
        acc += tmp * mask + (1.0 - mask) * 1.0                                     # lines 146-150
    out = float(acc.sum()) / (3 * 2)                                               # line 157
    return out * (3.0 / (3.0 * h * w)) if size_average else out


def lua_loss_ssim(table, ref, past, criterion="OSSIML1", flow_scale=TL.SCALE, like="test", size_average=False, weights=None, batch=True, alpha=None):
    """float64 array (n,): table_loss_fields.lua_loss with pme_criterion = nn.OSSIML1Criterion (model.lua:172-179).  Every other term is
    that function's (called with pme = 0); the photometric term is `ossiml1` per triplet with the range of the whole batch (batch=True:
    what the reference computes when the n triplets are one batch) or of the triplet alone."""
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    a = ALPHA[criterion] if alpha is None else alpha
    rest = dict(wt)
    rest["pme"] = 0.0
    out = TL.lua_loss(table, ref, past, flow_scale=flow_scale, like=like, size_average=size_average, weights=rest)
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    down = TL.ref_pyramid(ref, L)
    for l in range(L):
        lv = table[l * per:(l + 1) * per]
        for b in range(n):
            sel = slice(0, n) if batch else slice(b, b + 1)
            vals = [down[l][sel], lv[per - 2][sel], lv[per - 1][sel]]
            mn = float(min(float(v.min()) for v in vals))                          # lines 62-67
            mx = float(max(float(v.max()) for v in vals))
            sub = [t[b:b + 1] for t in lv]
            out[b] += TL.LEVEL_WEIGHTS[l] * wt["pme"] * ossiml1(sub, down[l][b:b + 1], past, flow_scale / 2.0 ** l, a, mn, mx, size_average)
    return out


def bound_ssim(H, W, L, past, alpha, like="test", size_average=False, weights=None, lua=0.0):
    """table_loss_fields.bound for the SSIM records: each q rounds by at most 2^-31 per counted pixel-direction, the summary weighs the
    two words by alpha and 1 - alpha and divides by 3 * 2, so the photometric part is level_weight * pme * (alpha + |1 - alpha|) *
    2 h w / 6 * 2^-31 (times 1 / (h w) with size_average): table_loss_fields.bound's own photometric part times alpha + |1 - alpha|, which
    is 1 for alpha in [0, 1].  Every other term is that function's."""
    assert 0.0 <= alpha <= 1.0
    return TL.bound(H, W, L, past, like=like, size_average=size_average, weights=weights, lua=lua)


def allowance_ssim(H, W, L, alpha, size_average=False, weights=None):
    """What the float64 evaluation of 1 - l cs may differ by between two correct evaluations in different orders (the library's separable
    window, the transcription's conv2d), derived and not measured; eps = 2^-53, all normalised values in [0, 1]:
      a window sum is a convex combination of at most nine values in [0, 1], evaluated with at most 17 rounded operations on rounded
      weights: within 20 eps of the exact sum.  A product of two of them: within 41 eps.  sigma = G(.) - mu mu: within 62 eps.
      l = N / D with D >= C1: N = 2 mu_x mu_y + C1 within 83 eps, D within 84 eps, |l| <= 1: l within 167 eps / C1 (+ its own rounding).
      cs = N / D with D >= C2 - 126 eps: N = 2 s_xy + C2 within 125 eps, D within 126 eps, |cs| <= 1 up to that error: cs within
      251 eps / C2.  1 - l cs: within the sum of the two, and one more eps; S sums three channels; o <= 1.
      The L1 part: P1 of a difference of two identical inputs, within 8 eps per channel.
    Two evaluations may lie that far on either side of the exact value, so a counted pixel-direction may differ by twice that; the
    summary scales it like the rounding bound: level_weight * pme * 2 h w / 6 per level (times 1 / (h w) with size_average)."""
    eps = 2.0 ** -53
    per_dir = 2.0 * (alpha * 3.0 * (167.0 * eps / C1 + 251.0 * eps / C2 + 2.0 * eps) + (1.0 - alpha) * 3.0 * 8.0 * eps)
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    total = 0.0
    for j in range(L):
        hw = float((H >> j) * (W >> j))
        total += TL.LEVEL_WEIGHTS[j] * wt["pme"] * (2.0 * hw / 6.0) * per_dir * ((1.0 / hw) if size_average else 1.0)
    return total
