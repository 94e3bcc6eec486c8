"""Shared by tests/test_table_loss_grad_cpu.py and tests/test_gpu_table_loss_grad.py: `want_grad`, the plain numpy restatement of
include/b2f.h's definition of the gradient table (`gradOutputs` of train.lua:428-468) that the host entry is held against bit for bit,
`lua_grad`, a float64 transcription of the reference's five updateGradInput functions and of the accumulation of train.lua:428-468, and
`torch_loss`, the forward criteria in torch float64 for autograd.  The tables are those of tests/table_loss_fields.py."""
import numpy as np

from back2future_amd import back2future
from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL

F32 = np.float32
TERMS = ("smooth_flow", "const_vel", "pme", "smooth_occ", "prior_occ")
DEFAULTS = {"smooth_flow": 1.0, "const_vel": 1.0, "pme": 1.0, "smooth_occ": 0.1, "prior_occ": 0.1,
            "level_weights": (0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28), "size_average": False}


def options(**kw):
    """the options as a dict: DEFAULTS with the keywords replaced"""
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def struct(o):
    """the dict as the b2f_loss_grad_opts the entries take"""
    wt = dict((k, o[k]) for k in TERMS)
    wt["level_weights"] = o["level_weights"]
    return back2future.loss_grad_options(weights=wt, size_average=o["size_average"])


def coefficients(o, j, h, w):
    """(k_s, k_cv, k_p, k_so, k_pr) of level j as include/b2f.h forms them"""
    c = float(o["level_weights"][j])
    n2 = 1.0 / ((2.0 * h) * w) if o["size_average"] else 1.0
    n1 = 1.0 / (float(h) * w) if o["size_average"] else 1.0
    return ((c * o["smooth_flow"]) * n2, (c * o["const_vel"]) * n1, ((c * o["pme"]) * n1) / 6.0, (c * o["smooth_occ"]) * n2,
            (c * o["prior_occ"]) * n1)


def _sum(terms, shape):
    """the enabled terms added left to right; +0.0 without one"""
    if not terms:
        return np.zeros(shape, np.float64)
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _shift(a, axis):
    """a(x - 1, y) (axis -1) or b(x, y - 1) (axis -2): 0 where there is no such pixel"""
    out = np.zeros_like(a)
    if axis == -1:
        out[..., :, 1:] = a[..., :, :-1]
    else:
        out[..., 1:, :] = a[..., :-1, :]
    return out


def want_grad(table, ref, past, flow_scale=TL.SCALE, o=None, with_mag=False):
    """the gradient table (float32 arrays with the table's shapes) by include/b2f.h's definition: fp64, one rounding to fp32.
    with_mag: also, per tensor, the sum of the magnitudes of the fp64 terms of every element (what the bar of lua_grad scales with)
    and the fp64 sums before the rounding"""
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    pyr = TL.ref_pyramid(ref, L)
    D1 = lambda v: v / np.sqrt(v * v + 1e-6)
    D2 = lambda v: 2.0 * v
    grads, mags = [], []
    with np.errstate(all="ignore"):
        for j in range(L):
            t = table[j * per:(j + 1) * per]
            f, p, oc, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
            R = pyr[j]
            n, _, h, w = R.shape
            k_s, k_cv, k_p, k_so, k_pr = coefficients(o, j, h, w)
            on = dict((k, o[k] != 0.0) for k in TERMS)
            rdx, rdy = TL._diffs(R)
            wx = TL.E(-20.0 * ((np.abs(rdx[:, 0]) + np.abs(rdx[:, 1])) + np.abs(rdx[:, 2])) / 3.0)[:, None]
            wy = TL.E(-20.0 * ((np.abs(rdy[:, 0]) + np.abs(rdy[:, 1])) + np.abs(rdy[:, 2])) / 3.0)[:, None]

            def S(F, D):
                dx, dy = TL._diffs(F)
                a, b = np.zeros_like(dx), np.zeros_like(dy)
                a[..., :, :-1] = (D(dx) * wx)[..., :, :-1]      # exactly 0 in the last column: no product there
                b[..., :-1, :] = (D(dy) * wy)[..., :-1, :]
                al, bu = _shift(a, -1), _shift(b, -2)
                return (((-a) + al) - b) + bu, ((np.abs(a) + np.abs(al)) + np.abs(b)) + np.abs(bu)

            shape2 = (n, 2, h, w)
            cv = None
            if past and on["const_vel"]:
                d = f.astype(np.float64) - p.astype(np.float64)
                den = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + 1e-12
                cv = d / den[:, None]
            sf = S(f, D1) if on["smooth_flow"] else None
            tf = ([k_s * sf[0]] if sf else []) + ([k_cv * cv] if cv is not None else [])
            g_f, m_f = _sum(tf, shape2), _sum(([abs(k_s) * sf[1]] if sf else []) + ([np.abs(k_cv * cv)] if cv is not None else []), shape2)
            if past:
                sp = S(p, D1) if on["smooth_flow"] else None
                tp = ([k_s * sp[0]] if sp else []) + ([-(k_cv * cv)] if cv is not None else [])
                g_p, m_p = _sum(tp, shape2), _sum(([abs(k_s) * sp[1]] if sp else []) + ([np.abs(k_cv * cv)] if cv is not None else []), shape2)
            po = np.zeros(shape2, np.float64)
            g_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            if on["pme"]:
                kd = float(F32(flow_scale / 2.0 ** j))
                for d in range(2):
                    fl = p if (d == 0 and past) else f
                    _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
                    m = inside & ~nan
                    delta = iw[d].astype(np.float64) - R.astype(np.float64)
                    s = np.sqrt(delta * delta + 1e-6)
                    e = (s[:, 0] + s[:, 1]) + s[:, 2]
                    po[:, 1 - d] = np.where(m, e, 1.0)
                    g_iw[d] = np.where(m[:, None], k_p * ((delta / s) * oc[:, 1 - d].astype(np.float64)[:, None]), 0.0)
            so = S(oc, D2) if on["smooth_occ"] else None
            pr = 1.0 - oc[:, ::-1].astype(np.float64) if on["prior_occ"] else None
            to = ([k_p * po] if on["pme"] else []) + ([k_so * so[0]] if so else []) + ([k_pr * pr] if pr is not None else [])
            mo = ([np.abs(k_p * po)] if on["pme"] else []) + ([abs(k_so) * so[1]] if so else []) + ([np.abs(k_pr * pr)] if pr is not None else [])
            g_o, m_o = _sum(to, shape2), _sum(mo, shape2)
            grads += [g_f] + ([g_p] if past else []) + [g_o, g_iw[0], g_iw[1]]
            mags += [m_f] + ([m_p] if past else []) + [m_o, np.abs(g_iw[0]), np.abs(g_iw[1])]
        out = [g.astype(F32) for g in grads]
    return (out, mags, grads) if with_mag else out


def lua_grad(table, ref, past, flow_scale=TL.SCALE, o=None):
    """`gradOutputs` per triplet in float64: criterions/SmoothnessCriterion.lua:75-106 (L1 penalty for flows, quadratic for
    occlusions), ConstVelCriterion.lua:48-74, OBCCriterion.lua:121-240 (L1 penalty, penalty_out = 1, 1-based fp32 target coordinates,
    pwc_flow_scaling = flow_scale / 2^l), OcclusionPriorCriterion.lua:51-73, accumulated as train.lua:428-468 does into zeroed
    tensors.  Each triplet is a batch of one, so sizeAverage's norms are per triplet."""
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    eps = 0.001 * 0.001
    l1 = lambda x: np.power(x * x + eps, 0.5)
    l1_der = lambda x: x / np.power(x * x + eps, 0.5)
    quad_der = lambda x: 2 * x
    down = TL.ref_pyramid(ref, L)
    avg = o["size_average"]
    out = [np.zeros(t.shape, np.float64) for t in table]

    def smoothness_back(inp, target, der):
        inp, target = inp.astype(np.float64), target.astype(np.float64)
        gy, gx, igy, igx = np.zeros_like(inp), np.zeros_like(inp), np.zeros_like(target), np.zeros_like(target)
        gy[:, :, :-1, :] = inp[:, :, 1:, :] - inp[:, :, :-1, :]
        gx[:, :, :, :-1] = inp[:, :, :, 1:] - inp[:, :, :, :-1]
        igy[:, :, :-1, :] = target[:, :, 1:, :] - target[:, :, :-1, :]
        igx[:, :, :, :-1] = target[:, :, :, 1:] - target[:, :, :, :-1]
        wy = np.exp(-20.0 * np.mean(np.abs(igy), axis=1, keepdims=True))
        wx = np.exp(-20.0 * np.mean(np.abs(igx), axis=1, keepdims=True))
        gy, gx = der(gy) * wy, der(gx) * wx
        gys1, gxs1 = np.zeros_like(inp), np.zeros_like(inp)
        gys1[:, :, 1:, :] = gy[:, :, :-1, :]
        gxs1[:, :, :, 1:] = gx[:, :, :, :-1]
        g = -gx + gxs1 - gy + gys1
        return (1.0 / inp.size) * g if avg else g

    def const_vel_back(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        npixels = a.size / a.shape[1]
        loss = np.sqrt(((a - b) ** 2).sum(axis=1, keepdims=True)) + 1e-12
        g1, g2 = (a - b) / loss, (b - a) / loss
        return (g1 / npixels, g2 / npixels) if avg else (g1, g2)

    def obcc_back(sub, target, scaling):
        warp_start = 3 if past else 2          # 0-based index of the first warped image
        occ = sub[warp_start - 1].astype(np.float64)
        _, _, h, w = sub[0].shape
        norm = 3.0 / (3.0 * h * w)
        cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
        cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
        g_occ = np.zeros_like(occ)
        g_img = []
        for f in (1, 2):
            img = sub[warp_start - 1 + f].astype(np.float64)
            buf = img - target.astype(np.float64)
            gi = l1_der(buf)
            buf = l1(buf).sum(axis=1)
            if f <= 1.0:
                fl = sub[1] if past else sub[0]
                tx = cx + (F32(f - 1 - 1) * fl[:, 0]) * F32(scaling)
                ty = cy + (F32(f - 1 - 1) * fl[:, 1]) * F32(scaling)
                ch = 1
            else:
                tx = cx + (F32(f - 1) * sub[0][:, 0]) * F32(scaling)
                ty = cy + (F32(f - 1) * sub[0][:, 1]) * F32(scaling)
                ch = 0
            mask = ((tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)).astype(np.float64)
            buf = buf * mask + (1.0 - mask) * 1.0
            gi = gi * mask[:, None]
            g_occ[:, ch] += buf
            gi = gi * occ[:, ch][:, None]
            gi = gi * (1.0 / (3 * 2))
            g_img.append(gi * norm if avg else gi)
        g_occ = g_occ * (1.0 / (3 * 2))
        return [g_occ * norm if avg else g_occ] + g_img

    def prior_back(occ):
        occ = occ.astype(np.float64)
        g = 1.0 - occ[:, ::-1]
        return g * (2.0 / occ.size) if avg else g

    with np.errstate(all="ignore"):
        for b in range(n):
            for l in range(L):
                sub = [t[b:b + 1] for t in table[l * per:(l + 1) * per]]
                dst = [g[b:b + 1] for g in out[l * per:(l + 1) * per]]
                target = down[l][b:b + 1]
                lw = o["level_weights"][l]
                for i in range(2 if past else 1):
                    dst[i] += lw * o["smooth_flow"] * smoothness_back(sub[i], target, l1_der)
                if past:
                    g1, g2 = const_vel_back(sub[0], sub[1])
                    dst[0] += lw * o["const_vel"] * g1
                    dst[1] += lw * o["const_vel"] * g2
                for i, v in enumerate(obcc_back(sub, target, flow_scale / 2.0 ** l)):
                    dst[per - 3 + i] += lw * o["pme"] * v
                if o["smooth_occ"] > 0:
                    dst[per - 3] += lw * o["smooth_occ"] * smoothness_back(sub[per - 3], target, quad_der)
                if o["prior_occ"] > 0:
                    dst[per - 3] += lw * o["prior_occ"] * prior_back(sub[per - 3])
    return out


def offset_past(table, seed=0):
    """the Soft table with every past flow replaced by the future flow plus an offset of magnitude 0.05 .. 0.5 at every pixel: the
    constant-velocity term has a derivative everywhere (autograd gives NaN at f == p)"""
    out = list(table)
    for j in range(len(table) // 5):
        f = table[5 * j]
        r = np.random.default_rng(seed * 31 + j)
        mag = r.uniform(0.05, 0.5, f[:, :1].shape)
        ang = r.uniform(0.0, 2.0 * np.pi, f[:, :1].shape)
        out[5 * j + 1] = (f + np.concatenate([mag * np.cos(ang), mag * np.sin(ang)], axis=1)).astype(F32)
    return out


def torch_loss(tensors, ref, past, flow_scale=TL.SCALE, o=None, cv_norm_of_gradient=False):
    """the objective of train.lua:428-468 as one torch float64 scalar, summed over the triplets (each a batch of one): the forward
    criteria SmoothnessCriterion.lua:28-73, ConstVelCriterion.lua:29-46, OBCCriterion.lua:36-119, OcclusionPriorCriterion.lua:28-49 on
    `tensors` (torch float64, the table).  The contrast weights and the inside masks are constants.  cv_norm_of_gradient: divide the
    constant-velocity output by h w as its updateGradInput does, not by 2 h w (quirk 3)."""
    import torch
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(tensors) // per
    avg = o["size_average"]
    down = TL.ref_pyramid(ref, L)
    total = 0.0
    for l in range(L):
        sub = tensors[l * per:(l + 1) * per]
        R = torch.from_numpy(down[l].astype(np.float64))
        n, _, h, w = R.shape
        lw = o["level_weights"][l]
        wx = torch.exp(-20.0 * (R[..., :, 1:] - R[..., :, :-1]).abs().mean(dim=1, keepdim=True))
        wy = torch.exp(-20.0 * (R[..., 1:, :] - R[..., :-1, :]).abs().mean(dim=1, keepdim=True))
        l1 = lambda x: torch.sqrt(x * x + 1e-6)

        def smooth(F, pen):
            # (the zero difference of the last column / row adds pen(0) * w there, a constant)
            s = (pen(F[..., :, 1:] - F[..., :, :-1]) * wx).sum() + (pen(F[..., 1:, :] - F[..., :-1, :]) * wy).sum()
            return s / (2.0 * h * w) if avg else s

        for i in range(2 if past else 1):
            total = total + lw * o["smooth_flow"] * smooth(sub[i], l1)
        if past:
            cv = torch.sqrt(((sub[0] - sub[1]) ** 2).sum(dim=1)).sum()
            total = total + lw * o["const_vel"] * (cv / ((1.0 if cv_norm_of_gradient else 2.0) * h * w) if avg else cv)
        occ = sub[per - 3]
        kd = float(F32(flow_scale / 2.0 ** l))
        acc = 0.0
        for d in range(2):
            fl = sub[1] if (d == 0 and past) else sub[0]
            _, _, nan, inside = FW.coordinates(fl.detach().numpy().astype(F32), -kd if d == 0 else kd)
            m = torch.from_numpy((inside & ~nan).astype(np.float64))
            e = l1(sub[per - 2 + d] - R).sum(dim=1) * occ[:, 1 - d]
            acc = acc + (e * m + (1.0 - m)).sum()
        acc = acc / 6.0
        total = total + lw * o["pme"] * (acc / (h * w) if avg else acc)
        total = total + lw * o["smooth_occ"] * smooth(occ, lambda x: x * x)
        pr = (1.0 - occ[:, 0] * occ[:, 1]).sum()
        total = total + lw * o["prior_occ"] * (pr / (h * w) if avg else pr)
    return total
