"""Shared by tests/test_table_loss_plain_cpu.py and tests/test_gpu_table_loss_plain.py: `want_plain`, the plain numpy restatement of
words 16 .. 29 of a record of the photometric terms without occlusion masking (include/b2f.h, B2F_LOSS_PLAIN_*), and `want_grad_plain`,
that of the gradient table of the *_grad_plain entries, which the host entries are held against bit for bit; `mbcc` / `mbcc_back` and
`mssiml1` / `mssiml1_back`, float64 transcriptions of criterions/MBCCriterion.lua and criterions/MSSIML1Criterion.lua written from the
Lua text (a 2-D kernel from the Gaussian formula, torch's replicate padding and conv2d, the range of `for i = 2,#input`) inside the
sums of train.lua:428-468 / test.lua:266-297 (`lua_loss_plain`, `lua_grad_plain`); and the bars between the two.  Everything the
definition takes over -- the tables, the first 16 words, the flow planes, S(o, D2), the coefficients, the window -- comes from the
existing helper modules."""
import numpy as np

from back2future_amd import back2future
from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL
from tests import table_loss_grad_fields as TG
from tests import table_loss_grad_ft_fields as TF
from tests import table_loss_grad_ssim as TGS
from tests import table_loss_ssim_fields as TS

F32 = np.float32
WORDS = 40
L1, SQ, SSIM, L1N, SSIM_NONFINITE, RANGE_USED, RANGE_OWN = 16, 18, 20, 22, 24, 26, 28
BATCH, IMAGE, GIVEN = TS.BATCH, TS.IMAGE, TS.GIVEN
ALPHA = {"SSIM": 1.0, "SSIML1": 0.85}        # model.lua:149-159
TERMS = TG.TERMS
DEFAULTS = dict(TG.DEFAULTS, smooth_second_order=False, pme_criterion="BCC", pme_penalty="L1", ssim_alpha=0.85)
# wrong readings of the Lua that the bit-for-bit tests must tell from the right one
MUTATIONS = ("occlusion_weight", "penalty_out", "range_images_only", "zero_padding", "quadratic_der")


def options(**kw):
    """the options as a dict: DEFAULTS with the keywords replaced; no_occ=True: the two occlusion weights at 0 (train.lua:456)"""
    o = dict(DEFAULTS)
    no_occ = kw.pop("no_occ", False)
    o.update(kw)
    if o["pme_criterion"] in ALPHA and "ssim_alpha" not in kw:
        o["ssim_alpha"] = ALPHA[o["pme_criterion"]]
    if no_occ:
        o["smooth_occ"] = o["prior_occ"] = 0.0
    return o


def struct(o):
    """the dict as the b2f_loss_grad_plain_opts the entries take"""
    wt = dict((k, o[k]) for k in TERMS)
    wt["level_weights"] = o["level_weights"]
    ssim = o["pme_criterion"] != "BCC"
    return back2future.loss_grad_plain_options(weights=wt, size_average=o["size_average"], smooth_second_order=o["smooth_second_order"],
                                               pme_criterion=o["pme_criterion"], pme_penalty=o["pme_penalty"],
                                               ssim_alpha=o["ssim_alpha"] if ssim else None)


range_arg = TGS.range_arg


def range_planes(R, t, past):
    """the tensors MSSIML1Criterion.lua:63-68 takes the minimum and maximum over: y and input[2 ..] -- on a Hard table the occlusions
    and the warped images, on a Soft one the past flow as well"""
    per = 5 if past else 4
    return [R, t[per - 2], t[per - 1], t[per - 3]] + ([t[1]] if past else [])


def used_bits(R, t, past, mode, ranges, j, L, images_only=False):
    """per image: ((own mn bits, own mx bits), (used mn bits, used mx bits)) at level j"""
    n = R.shape[0]
    per = 5 if past else 4
    planes = [R, t[per - 2], t[per - 1]] if images_only else range_planes(R, t, past)
    own = [TS.own_range_bits([p[b] for p in planes]) for b in range(n)]
    if mode == BATCH:
        used = [TS.own_range_bits(planes)] * n
    elif mode == IMAGE:
        used = own
    else:
        g = np.asarray(ranges, F32).reshape(L, 2)[j].view(np.uint32)
        used = [(g[0], g[1])] * n
    return own, used


def _counted(fl, kd_signed, delta, wt):
    """(inside, PHOTO_INSIDE) of a direction: the target's inside test, and with it no NaN in the coordinate, the L1 sum or the weight"""
    _, _, nan, inside = FW.coordinates(fl, kd_signed)
    s = np.sqrt(delta * delta + 1e-6)
    e = (s[:, 0] + s[:, 1]) + s[:, 2]
    we = wt * e
    return inside & ~nan, inside & ~(nan | np.isnan(e) | np.isnan(we) | np.isnan(wt)), e


def want_plain(table, ref, past, flow_scale=TL.SCALE, mode=BATCH, ranges=None, mutation=None):
    """uint64 (n, L, 14): words 16 .. 29 by the definition of include/b2f.h, one expression per word.  mutation: one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    pyr = TL.ref_pyramid(ref, L)
    ge, gc = TS.weights()
    zp = mutation == "zero_padding"
    rec = np.zeros((n, L, 14), np.uint64)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    for j in range(L):
        t = table[j * per:(j + 1) * per]
        f, p, o, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
        R = pyr[j]
        own, used = used_bits(R, t, past, mode, ranges, j, L, mutation == "range_images_only")
        kd = float(F32(flow_scale / 2.0 ** j))
        for b in range(n):
            rec[b, j, RANGE_OWN - 16], rec[b, j, RANGE_OWN - 15] = own[b]
            rec[b, j, RANGE_USED - 16], rec[b, j, RANGE_USED - 15] = used[b]
            mn, mx = TS._as_float(used[b][0]), TS._as_float(used[b][1])
            ok = bool(mx > mn) and bool(np.isfinite(mn)) and bool(np.isfinite(mx))
            with np.errstate(all="ignore"):
                norm = lambda a: (a[b:b + 1].astype(np.float64) - np.float64(mn)) / (np.float64(mx) - np.float64(mn))
                y = norm(R)
                mu_y = TS._window(y, ge, gc, zp)
                s_y = TS._window(y * y, ge, gc, zp) - mu_y * mu_y
            for d in range(2):
                fl = p if (d == 0 and past) else f
                with np.errstate(all="ignore"):
                    delta = iw[d][b:b + 1].astype(np.float64) - R[b:b + 1].astype(np.float64)
                    wt = o[b:b + 1, 1 - d].astype(np.float64)
                    m, counted, B1 = _counted(fl[b:b + 1], -kd if d == 0 else kd, delta, wt)
                    q = delta * delta
                    B2 = (q[:, 0] + q[:, 1]) + q[:, 2]
                    x = norm(iw[d])
                    mu_x = TS._window(x, ge, gc, zp)
                    s_x = TS._window(x * x, ge, gc, zp) - mu_x * mu_x
                    s_xy = TS._window(x * y, ge, gc, zp) - mu_x * mu_y
                    l = (2.0 * (mu_x * mu_y) + 1e-4) / ((mu_x * mu_x + mu_y * mu_y) + 1e-4)
                    cs = (2.0 * s_xy + 9e-4) / ((s_x + s_y) + 9e-4)
                    one = 1.0 - l * cs
                    S = (one[:, 0] + one[:, 1]) + one[:, 2]
                    pd = P1(x - y)
                    B = (pd[:, 0] + pd[:, 1]) + pd[:, 2]
                    if mutation == "occlusion_weight":
                        B1, B2, S, B = wt * B1, wt * B2, wt * S, wt * B
                out = np.uint64((~m).sum() << 30) if mutation == "penalty_out" else np.uint64(0)
                rec[b, j, L1 - 16 + d] = TL._q30_sum(np.where(counted, B1, 0.0), counted)[0] + out
                rec[b, j, SQ - 16 + d] = TL._q30_sum(np.where(counted, B2, 0.0), counted)[0] + out
                if not ok:
                    rec[b, j, SSIM_NONFINITE - 16 + d] = counted.sum()
                    continue
                nonf = counted & (np.isnan(S) | np.isnan(B))
                good = counted & ~nonf
                rec[b, j, SSIM - 16 + d] = TL._q30_sum(np.where(good, S, 0.0), good)[0] + out
                rec[b, j, L1N - 16 + d] = TL._q30_sum(np.where(good, B, 0.0), good)[0] + out
                rec[b, j, SSIM_NONFINITE - 16 + d] = nonf.sum()
    return rec


def want_grad_plain(table, ref, past, flow_scale=TL.SCALE, o=None, mode=BATCH, ranges=None, mutation=None, with_mag=False):
    """the gradient table (float32 arrays with the table's shapes) by include/b2f.h's definition: fp64, one rounding to fp32.
    mutation: one of MUTATIONS.  with_mag: also, per tensor, the magnitudes the bar of lua_grad_plain scales with (as
    tests/table_loss_grad_ssim.want_grad_ssim counts them; the flow planes: None), and the fp64 sums before the rounding"""
    assert mutation is None or mutation in MUTATIONS
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    pyr = TL.ref_pyramid(ref, L)
    ge, gc = TS.weights()
    zp = mutation == "zero_padding"
    ssim = o["pme_criterion"] != "BCC"
    alpha = float(o["ssim_alpha"])
    beta = 1.0 - alpha
    D1 = lambda v: v / np.sqrt(v * v + 1e-6)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    G = lambda a: TS._window(a, ge, gc, zp)
    flows, _, flows64 = TF.want_grad_ft(table, ref, past, flow_scale, TGS.ft_options(o, pme=0.0), with_mag=True)
    on = dict((k, o[k] != 0.0) for k in TERMS)
    so64 = None
    if on["smooth_occ"]:
        so64 = TF.want_grad_ft(table, ref, past, flow_scale, TGS.ft_options(o, smooth_flow=0.0, const_vel=0.0, pme=0.0, prior_occ=0.0), with_mag=True)[2]
    grads, mags = [], []
    with np.errstate(all="ignore"):
        for j in range(L):
            t = table[j * per:(j + 1) * per]
            f, p, oc, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
            R = pyr[j]
            n, _, h, w = R.shape
            _, _, k_p, k_so, k_pr = TG.coefficients(o, j, h, w)
            shape2 = (n, 2, h, w)
            g_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            m_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            po = np.zeros(shape2, np.float64)
            if on["pme"]:
                kd = float(F32(flow_scale / 2.0 ** j))
                if ssim:
                    _, used = used_bits(R, t, past, mode, ranges, j, L, mutation == "range_images_only")
                    mn = np.array([TS._as_float(u[0]) for u in used], np.float64).reshape(n, 1, 1, 1)
                    mx = np.array([TS._as_float(u[1]) for u in used], np.float64).reshape(n, 1, 1, 1)
                    norm = lambda a: (a.astype(np.float64) - mn) / (mx - mn)
                    y = norm(R)
                    mu_y, gyy = G(y), G(y * y)
                    gw = gc * gc
                for d in range(2):
                    fl = p if (d == 0 and past) else f
                    _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
                    m = inside & ~nan
                    if ssim:
                        x = norm(iw[d])
                        mu_x = G(x)
                        gxx, gxy = G(x * x), G(x * y)
                        xx, yy, xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
                        s_x, s_y, s_xy = gxx - xx, gyy - yy, gxy - xy
                        A, Bd = (xx + yy) + 1e-4, (s_x + s_y) + 9e-4
                        l, cs = (2.0 * xy + 1e-4) / A, (2.0 * s_xy + 9e-4) / Bd
                        dl = ((2.0 * gw) * (mu_y - mu_x * l)) / A
                        dcs = ((2.0 * gw) * ((y - mu_y) - cs * (x - mu_x))) / Bd
                        Q = dl * cs + l * dcs
                        mQ = np.abs((2.0 * gw) * (np.abs(mu_y) + np.abs(mu_x)) / A) + np.abs((2.0 * gw) * ((np.abs(y) + np.abs(mu_y)) + (np.abs(x) + np.abs(mu_x))) / Bd)
                        terms, tm = [], []
                        if alpha != 0.0:
                            terms.append(-(alpha * Q))
                            tm.append(alpha * mQ)
                        if beta != 0.0:
                            terms.append(beta * D1(x - y))
                            tm.append(np.abs(beta * D1(x - y)))
                        T, Tm = TG._sum(terms, x.shape), TG._sum(tm, x.shape)
                    else:
                        delta = iw[d].astype(np.float64) - R.astype(np.float64)
                        if o["pme_penalty"] == "Quadratic":
                            T = delta if mutation == "quadratic_der" else 2.0 * delta
                        else:
                            T = D1(delta)
                        Tm = np.abs(T)
                    if mutation == "occlusion_weight":
                        T = T * oc[:, 1 - d].astype(np.float64)[:, None]
                    g_iw[d] = np.where(m[:, None], k_p * T, 0.0)
                    m_iw[d] = np.where(m[:, None], np.abs(k_p * Tm), 0.0)
                    if mutation == "penalty_out":
                        po[:, 1 - d] = np.where(m, 0.0, 1.0)
            pr = 1.0 - oc[:, ::-1].astype(np.float64) if on["prior_occ"] else None
            so = so64[j * per + per - 3] if on["smooth_occ"] else None
            to = ([k_p * po] if (mutation == "penalty_out" and on["pme"]) else []) + ([so] if so is not None else []) + ([k_pr * pr] if pr is not None else [])
            mo = ([np.abs(so)] if so is not None else []) + ([np.abs(k_pr * pr)] if pr is not None else [])
            g_o, m_o = TG._sum(to, shape2), TG._sum(mo, shape2)
            grads += [flows64[j * per]] + ([flows64[j * per + 1]] if past else []) + [g_o, g_iw[0], g_iw[1]]
            mags += [None] + ([None] if past else []) + [m_o, m_iw[0], m_iw[1]]
        out = [g.astype(F32) for g in grads]
    for j in range(L):      # the flow planes: want_grad_ft's own rounding
        for i in range(2 if past else 1):
            out[j * per + i] = flows[j * per + i]
    return (out, mags, grads) if with_mag else out


# ---- the transcriptions: written from the Lua text, torch float64, sharing nothing with the restatement's photometric part ----

def _targets(sub, past, f, scaling, h, w):
    """the 1-based fp32 target coordinates of frame f (1: past, 2: future) and their mask (MBCCriterion.lua:70-87)"""
    cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
    cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
    if f <= 1.0:
        fl = sub[1] if past else sub[0]
        tx = cx + (F32(f - 1 - 1) * fl[:, 0]) * F32(scaling)
        ty = cy + (F32(f - 1 - 1) * fl[:, 1]) * F32(scaling)
    else:
        tx = cx + (F32(f - 1) * sub[0][:, 0]) * F32(scaling)
        ty = cy + (F32(f - 1) * sub[0][:, 1]) * F32(scaling)
    with np.errstate(all="ignore"):
        return ((tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)).astype(np.float64)


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _penalty(name):
    """(apply, der) of criterions/penalty: L1_function.lua (eps = 0.001) or quadratic_function.lua"""
    import torch
    if name == "Quadratic":
        return (lambda x: x * x), (lambda x: 2 * x)
    return (lambda x: torch.sqrt(x * x + 0.001 * 0.001)), (lambda x: x / torch.sqrt(x * x + 0.001 * 0.001))


def mbcc(sub, target, past, scaling, penalty, size_average, tensors=None):
    """MBCCriterion:updateOutput on one triplet (lines 35-102) in torch float64; tensors: the two warped images as torch tensors
    (for autograd), else taken from sub"""
    import torch
    warp_start = 3 if past else 2
    _, _, h, w = sub[0].shape
    apply, _ = _penalty(penalty)
    acc = torch.zeros(1, h, w, dtype=torch.float64)
    for f in (1, 2):
        img = tensors[f - 1] if tensors is not None else _T(sub[warp_start - 1 + f])
        buffer = apply(img - _T(target)).sum(1)                                    # lines 65-66
        acc = acc + buffer * torch.from_numpy(_targets(sub, past, f, scaling, h, w))   # lines 84-92
    out = acc.sum() / (3 * 2)                                                      # line 96
    return out * (3.0 / (3.0 * h * w)) if size_average else out


def mbcc_back(sub, target, past, scaling, penalty, size_average):
    """MBCCriterion:updateGradInput on one triplet (lines 104-186) -> [g_occ, g_img1, g_img2] as numpy float64"""
    import torch
    warp_start = 3 if past else 2
    _, _, h, w = sub[0].shape
    norm = 3.0 / (3.0 * h * w)                                                     # line 128
    _, der = _penalty(penalty)
    out = [np.zeros(sub[warp_start - 1].shape, np.float64)]                        # line 136
    for f in (1, 2):
        buffer = _T(sub[warp_start - 1 + f]) - _T(target)                          # line 146
        gi = der(buffer) * torch.from_numpy(_targets(sub, past, f, scaling, h, w))[:, None]   # lines 149, 167-175
        gi = gi * (1.0 / (3 * 2))                                                  # line 179
        out.append((gi * norm if size_average else gi).numpy())
    return out


def _conv():
    import torch
    import torch.nn.functional as F
    weight = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
    for c in range(3):
        weight[c, c] = torch.from_numpy(TS.gaussian3())                            # lines 36-42
    return lambda a: F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), weight)


def lua_range(sub_batch, target_batch):
    """(mn, mx) of MSSIML1Criterion.lua:63-68: over y and input[2 ..]"""
    vals = [target_batch] + list(sub_batch[1:])
    return float(min(float(v.min()) for v in vals)), float(max(float(v.max()) for v in vals))


def mssiml1(sub, target, past, scaling, alpha, mn, mx, size_average, tensors=None, own_window_of=None):
    """MSSIML1Criterion:updateOutput on one triplet (lines 45-153) in torch float64.  tensors: the warped images as torch tensors.
    own_window_of=(f, c, y, x): only that pixel's own window term of frame f, channel c (what lines 218-224 differentiate)."""
    import torch
    conv = _conv()
    warp_start = 3 if past else 2
    _, _, h, w = sub[0].shape
    y = (_T(target) - mn) / (mx - mn)                                              # line 74
    mu_y = conv(y)                                                                 # lines 89-90
    sigma_y = conv(y ** 2) - mu_y ** 2
    acc = torch.zeros(1, h, w, dtype=torch.float64)
    for f in (1, 2):
        raw = tensors[f - 1] if tensors is not None else _T(sub[warp_start - 1 + f])
        img = (raw - mn) / (mx - mn)                                               # line 100
        buffer = img - y                                                           # line 105
        mu_x = conv(img)                                                           # lines 108-110
        sigma_x = conv(img ** 2) - mu_x ** 2
        sigma_xy = conv(img * y) - mu_x * mu_y
        ssim_l = (2 * mu_x * mu_y + TS.C1) / (mu_x ** 2 + mu_y ** 2 + TS.C1)       # lines 113-114
        ssim_cs = (2 * sigma_xy + TS.C2) / (sigma_x + sigma_y + TS.C2)
        if own_window_of is not None:
            ff, c, yy, xx = own_window_of
            if ff == f:
                return alpha * (1 - ssim_l * ssim_cs)[0, c, yy, xx] + (1 - alpha) * torch.sqrt(buffer * buffer + 0.001 * 0.001)[0, c, yy, xx]
            continue
        tmp = alpha * (1 - ssim_l * ssim_cs).sum(1) + (1 - alpha) * torch.sqrt(buffer * buffer + 0.001 * 0.001).sum(1)   # line 117
        acc = acc + tmp * torch.from_numpy(_targets(sub, past, f, scaling, h, w))  # lines 135-143
    out = acc.sum() / (3 * 2)                                                      # line 147
    return out * (3.0 / (3.0 * h * w)) if size_average else out


def mssiml1_back(sub, target, past, scaling, alpha, mn, mx, size_average, masked=True):
    """MSSIML1Criterion:updateGradInput on one triplet (lines 155-261) -> [g_occ, g_img1, g_img2] as numpy float64"""
    import torch
    conv = _conv()
    kernel = torch.from_numpy(TS.gaussian3())
    warp_start = 3 if past else 2
    _, _, h, w = sub[0].shape
    norm = 3.0 / (3.0 * h * w)                                                     # line 181
    y = (_T(target) - mn) / (mx - mn)
    mu_y = conv(y)
    sigma_y = conv(y ** 2) - mu_y ** 2
    out = [np.zeros(sub[warp_start - 1].shape, np.float64)]                        # line 194
    for f in (1, 2):
        img = (_T(sub[warp_start - 1 + f]) - mn) / (mx - mn)                       # line 199
        buffer = img - y                                                           # line 204
        mu_x = conv(img)                                                           # lines 209-211
        sigma_x = conv(img ** 2) - mu_x ** 2
        sigma_xy = conv(img * y) - mu_x * mu_y
        ssim_l = (2 * mu_x * mu_y + TS.C1) / (mu_x ** 2 + mu_y ** 2 + TS.C1)       # lines 214-215
        ssim_cs = (2 * sigma_xy + TS.C2) / (sigma_x + sigma_y + TS.C2)
        gw = kernel[1, 1]                                                          # line 218
        d_l = 2 * gw * ((mu_y - mu_x * ssim_l) / (mu_x ** 2 + mu_y ** 2 + TS.C1))  # line 219
        d_cs = 2 * gw * (((y - mu_y) - ssim_cs * (img - mu_x)) / (sigma_x + sigma_y + TS.C2))   # line 220
        gi = -alpha * (d_l * ssim_cs + ssim_l * d_cs) + (1 - alpha) * (buffer / torch.sqrt(buffer * buffer + 0.001 * 0.001))   # line 224
        if masked:
            gi = gi * torch.from_numpy(_targets(sub, past, f, scaling, h, w))[:, None]   # lines 242-250
        gi = gi * (1.0 / (3 * 2))                                                  # line 254
        out.append((gi * norm if size_average else gi).numpy())
    return out


def lua_loss_plain(table, ref, past, criterion="BCC", penalty="L1", flow_scale=TL.SCALE, like="test", size_average=False, weights=None, batch=True,
                   alpha=None, no_occ=False):
    """float64 array (n,): table_loss_fields.lua_loss with pme_criterion = nn.MBCCriterion or nn.MSSIML1Criterion (model.lua:149-159).
    Every other term is that function's (called with pme = 0, and with no_occ the two occlusion weights 0: train.lua:456, test.lua:289);
    the range of MSSIML1 is that of the whole batch or of the triplet alone."""
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    if no_occ:
        wt["smooth_occ"] = wt["prior_occ"] = 0.0
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
            sub = [t[b:b + 1] for t in lv]
            tgt = down[l][b:b + 1]
            if criterion == "BCC":
                v = float(mbcc(sub, tgt, past, flow_scale / 2.0 ** l, penalty, size_average))
            else:
                sel = slice(0, n) if batch else slice(b, b + 1)
                mn, mx = lua_range([t[sel] for t in lv], down[l][sel])
                v = float(mssiml1(sub, tgt, past, flow_scale / 2.0 ** l, ALPHA[criterion] if alpha is None else alpha, mn, mx, size_average))
            out[b] += TL.LEVEL_WEIGHTS[l] * wt["pme"] * v
    return out


def lua_grad_plain(table, ref, past, flow_scale=TL.SCALE, o=None, ranges=None):
    """`gradOutputs` per triplet in float64: tests/table_loss_grad_ft_fields.lua_grad_ft for every criterion but the photometric one,
    and MBCCriterion / MSSIML1Criterion:updateGradInput with the range of the whole batch or, with ranges (L x 2), the given one;
    accumulated as train.lua:428-468 does"""
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    out = TF.lua_grad_ft(table, ref, past, flow_scale, TGS.ft_options(o, pme=0.0))
    down = TL.ref_pyramid(ref, L)
    with np.errstate(all="ignore"):
        for l in range(L):
            lv = table[l * per:(l + 1) * per]
            if o["pme_criterion"] != "BCC":
                mn, mx = lua_range(lv, down[l]) if ranges is None else (float(F32(ranges[l][0])), float(F32(ranges[l][1])))
            for b in range(n):
                sub = [t[b:b + 1] for t in lv]
                dst = [g[b:b + 1] for g in out[l * per:(l + 1) * per]]
                if o["pme_criterion"] == "BCC":
                    back = mbcc_back(sub, down[l][b:b + 1], past, flow_scale / 2.0 ** l, o["pme_penalty"], o["size_average"])
                else:
                    back = mssiml1_back(sub, down[l][b:b + 1], past, flow_scale / 2.0 ** l, o["ssim_alpha"], mn, mx, o["size_average"])
                for i, v in enumerate(back):
                    dst[per - 3 + i] += o["level_weights"][l] * o["pme"] * v
    return out


def bound_plain(H, W, L, past, criterion, alpha=None, like="test", size_average=False, weights=None, lua=0.0, no_occ=False):
    """The bar of loss_summary against lua_loss_plain.  The records' part is table_loss_fields.bound's: each q rounds by at most 2^-31
    per counted pixel-direction, the summary divides the two directions' sums by 3 * 2 (for SSIM / SSIML1 the two words are weighed
    alpha and 1 - alpha, which add to 1: bound_ssim).  The fp64 part: for BCC both sides evaluate the same three roots and two adds
    per pixel-direction, within 1e-12 of the value (bound's `lua` term); for SSIM / SSIML1 allowance_ssim of the existing helpers,
    which was derived with the factor o <= 1 counted as 1 and so applies unchanged without it."""
    wt = dict(TL.WEIGHTS)
    wt.update(weights or {})
    if no_occ:
        wt["smooth_occ"] = wt["prior_occ"] = 0.0
    if criterion == "BCC":
        return TL.bound(H, W, L, past, like=like, size_average=size_average, weights=wt, lua=lua)
    a = ALPHA[criterion] if alpha is None else alpha
    return TS.bound_ssim(H, W, L, past, a, like=like, size_average=size_average, weights=wt, lua=lua) + TS.allowance_ssim(H, W, L, a, size_average, wt)


def allowance_bcc_grad():
    """`a` of the bar 2^-24 |v| + 2^-149 + a m between want_grad_plain and lua_grad_plain for the image planes of BCC, counted in
    roundings of the element's magnitude m = |v|, eps = 2^-53.  Both sides form delta alike (one fp64 subtraction of two fp32 values,
    exact).  The restatement: D1 = delta / sqrt(delta delta + 1e-6), 4 roundings (2 delta: none); k_p = ((c pme) n1) / 6 with n1 = 1 /
    (h w), 4; their product, 1: 9.  The transcription: D1, 4, with the constant 0.001 * 0.001, which is 1e-6 (1 + 2 eps), half of which
    reaches D1: 1; times 1 / 6, itself rounded, 2; times norm = 3 / (3 h w), 2; times (c pme), 2: 11.  Together 20; 24 is asked."""
    return 24.0 * 2.0 ** -53
