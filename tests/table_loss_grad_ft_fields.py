"""Shared by tests/test_table_loss_grad_ft_cpu.py and tests/test_gpu_table_loss_grad_ft.py: `want_grad_ft`, the plain numpy restatement
of include/b2f.h's definition of the gradient table of the Soft models' fine-tuning objective (the *_grad_ft entries) that the host entry
is held against bit for bit, `lua_grad_ft`, a float64 transcription of criterions/SecondOrderSmoothnessCriterion.lua:77-104 and
criterions/OBGCCriterion.lua:151-300 beside the first-order functions and of the accumulation of train.lua:428-468, and `torch_terms`, the
two forward criteria in torch float64 for autograd.  The tables are those of tests/table_loss_fields.py."""
import numpy as np

from back2future_amd import back2future
from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL
from tests import table_loss_grad_fields as TG

F32 = np.float32
TERMS = TG.TERMS
FT_KEYS = ("smooth_second_order", "pme_criterion", "pme_alpha", "pme_beta", "pme_gamma")
DEFAULTS = dict(TG.DEFAULTS, smooth_second_order=True, pme_criterion="OBGCC", pme_alpha=1.0, pme_beta=1.0, pme_gamma=1.0)
# the eight weights of which a zero switches a term off
WEIGHTS8 = TERMS + ("pme_alpha", "pme_beta", "pme_gamma")


def options(**kw):
    """the options as a dict: DEFAULTS with the keywords replaced"""
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def objective(name, **kw):
    """the options of LOSS_OBJECTIVES[name] as a dict"""
    ob = back2future.LOSS_OBJECTIVES[name]
    o = options(**dict((k, ob[k]) for k in FT_KEYS))
    o.update(ob["weights"])
    o.update(kw)
    return o


def struct(o):
    """the dict as the b2f_loss_grad_ft_opts the entries take"""
    wt = dict((k, o[k]) for k in TERMS)
    wt["level_weights"] = o["level_weights"]
    return back2future.loss_grad_ft_options(weights=wt, size_average=o["size_average"], **dict((k, o[k]) for k in FT_KEYS))


def first_order(o):
    """the dict without the fine-tuning keys: the options of tests/table_loss_grad_fields.py"""
    return dict((k, v) for k, v in o.items() if k not in FT_KEYS)


def _shift_next(a, axis):
    """a(x + 1, y) (axis -1) or a(x, y + 1) (axis -2): 0 where there is no such pixel"""
    out = np.zeros_like(a)
    if axis == -1:
        out[..., :, :-1] = a[..., :, 1:]
    else:
        out[..., :-1, :] = a[..., 1:, :]
    return out


def _interior(h, w):
    """(ix, iy): h x w masks of the pixels with both neighbours on the axis"""
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    return np.broadcast_to((x >= 1) & (x + 1 < w), (h, w)), np.broadcast_to((y >= 1) & (y + 1 < h), (h, w))


def want_grad_ft(table, ref, past, flow_scale=TL.SCALE, o=None, with_mag=False):
    """the gradient table (float32 arrays with the table's shapes) by include/b2f.h's definition: fp64, one rounding to fp32.
    with_mag: also, per tensor, (m, mt): m the sum of the magnitudes of the fp64 terms of every element, mt the same sum with every
    term that carries a contrast weight E(t) scaled by 1 + |t| / 2 (what the bar of lua_grad_ft scales with), and the fp64 sums before
    the rounding"""
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    pyr = TL.ref_pyramid(ref, L)
    D1 = lambda v: v / np.sqrt(v * v + 1e-6)
    D2 = lambda v: 2.0 * v
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    second, obgcc = bool(o["smooth_second_order"]), o["pme_criterion"] == "OBGCC"
    alpha, beta, gamma = float(o["pme_alpha"]), float(o["pme_beta"]), float(o["pme_gamma"])
    grads, mags = [], []
    with np.errstate(all="ignore"):
        for j in range(L):
            t = table[j * per:(j + 1) * per]
            f, p, oc, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
            R = pyr[j]
            n, _, h, w = R.shape
            k_s, k_cv, k_p, k_so, k_pr = TG.coefficients(o, j, h, w)
            on = dict((k, o[k] != 0.0) for k in TERMS)
            rdx, rdy = TL._diffs(R)
            ax = ((np.abs(rdx[:, 0]) + np.abs(rdx[:, 1])) + np.abs(rdx[:, 2]))[:, None]     # the pair (x, y), (x + 1, y)
            ay = ((np.abs(rdy[:, 0]) + np.abs(rdy[:, 1])) + np.abs(rdy[:, 2]))[:, None]
            tx, ty = -20.0 * ax / 3.0, -20.0 * ay / 3.0
            wx, wy = TL.E(tx), TL.E(ty)
            ix, iy = _interior(h, w)
            t2x = -20.0 * (TG._shift(ax, -1) / 3.0 + ax / 3.0)                               # m((x,y), (x-1,y)) + m((x,y), (x+1,y))
            t2y = -20.0 * (TG._shift(ay, -2) / 3.0 + ay / 3.0)
            w2x, w2y = TL.E(t2x), TL.E(t2y)

            def S(F, D):
                dx, dy = TL._diffs(F)
                a, b = np.zeros_like(dx), np.zeros_like(dy)
                a[..., :, :-1] = (D(dx) * wx)[..., :, :-1]      # exactly 0 in the last column: no product there
                b[..., :-1, :] = (D(dy) * wy)[..., :-1, :]
                al, bu = TG._shift(a, -1), TG._shift(b, -2)
                sa, sb = np.abs(a) * (1.0 + np.abs(tx) / 2.0), np.abs(b) * (1.0 + np.abs(ty) / 2.0)
                return ((((-a) + al) - b) + bu, ((np.abs(a) + np.abs(al)) + np.abs(b)) + np.abs(bu),
                        ((sa + TG._shift(sa, -1)) + sb) + TG._shift(sb, -2))

            def S2(F):
                F = F.astype(np.float64)
                gx, gy = np.zeros_like(F), np.zeros_like(F)
                gx[..., :, 1:-1] = (2.0 * F[..., :, 1:-1] - F[..., :, :-2]) - F[..., :, 2:]
                gy[..., 1:-1, :] = (2.0 * F[..., 1:-1, :] - F[..., :-2, :]) - F[..., 2:, :]
                qx = np.where(ix, D1(gx) * w2x, 0.0)            # not formed off the interior: +0.0
                qy = np.where(iy, D1(gy) * w2y, 0.0)
                qyd, qxr, qyu, qxl = _shift_next(qy, -2), _shift_next(qx, -1), TG._shift(qy, -2), TG._shift(qx, -1)
                val = (((((2.0 * qy) + (2.0 * qx)) - qyd) - qxr) - qyu) - qxl
                m = lambda ay_, ax_: ((((2.0 * ay_ + 2.0 * ax_) + _shift_next(ay_, -2)) + _shift_next(ax_, -1)) + TG._shift(ay_, -2)) + TG._shift(ax_, -1)
                sx = np.abs(qx) * (1.0 + np.where(ix, np.abs(t2x), 0.0) / 2.0)
                sy = np.abs(qy) * (1.0 + np.where(iy, np.abs(t2y), 0.0) / 2.0)
                return val, m(np.abs(qy), np.abs(qx)), m(sy, sx)

            SF = S2 if second else (lambda F: S(F, D1))
            shape2 = (n, 2, h, w)
            zero2 = np.zeros(shape2, np.float64)
            cv = None
            if past and on["const_vel"]:
                d = f.astype(np.float64) - p.astype(np.float64)
                den = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + 1e-12
                cv = d / den[:, None]
            cvm = [np.abs(k_cv * cv)] if cv is not None else []
            sf = SF(f) if on["smooth_flow"] else None
            g_f = TG._sum(([k_s * sf[0]] if sf else []) + ([k_cv * cv] if cv is not None else []), shape2)
            m_f = (TG._sum(([abs(k_s) * sf[1]] if sf else []) + cvm, shape2), abs(k_s) * sf[2] if sf else zero2)
            if past:
                sp = SF(p) if on["smooth_flow"] else None
                g_p = TG._sum(([k_s * sp[0]] if sp else []) + ([-(k_cv * cv)] if cv is not None else []), shape2)
                m_p = (TG._sum(([abs(k_s) * sp[1]] if sp else []) + cvm, shape2), abs(k_s) * sp[2] if sp else zero2)
            po, pom = np.zeros(shape2, np.float64), np.zeros(shape2, np.float64)
            g_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            m_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            if on["pme"]:
                kd = float(F32(flow_scale / 2.0 ** j))
                has_u = np.broadcast_to(np.arange(h)[:, None] > 0, (h, w))
                has_l = np.broadcast_to(np.arange(w)[None, :] > 0, (h, w))

                def T(Fn, delta, ey, ex):
                    """the enabled terms left to right; Fn maps the errors of all three channels to what is weighted; (sum, magnitudes)"""
                    terms = []      # (term, where it is present or None)
                    if alpha != 0.0:
                        terms.append((alpha * Fn(delta), None))
                    if gamma != 0.0:
                        v = Fn(ey)
                        terms += [(-(gamma * v), None), (gamma * TG._shift(v, -2), has_u)]
                    if beta != 0.0:
                        v = Fn(ex)
                        terms += [(-(beta * v), None), (beta * TG._shift(v, -1), has_l)]
                    if not terms:
                        z = np.zeros(Fn(delta).shape, np.float64)
                        return z, z
                    acc, mag = terms[0][0], np.abs(terms[0][0])
                    for v, present in terms[1:]:
                        acc = acc + v if present is None else np.where(present, acc + v, acc)
                        mag = mag + np.abs(v) if present is None else np.where(present, mag + np.abs(v), mag)
                    return acc, mag

                for d in range(2):
                    fl = p if (d == 0 and past) else f
                    _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
                    m = inside & ~nan
                    o64 = oc[:, 1 - d].astype(np.float64)[:, None]
                    delta = iw[d].astype(np.float64) - R.astype(np.float64)
                    if obgcc:
                        idx, idy = TL._diffs(iw[d])
                        ex, ey = idx - rdx, idy - rdy
                        timg, mimg = T(D1, delta, ey, ex)
                        P3 = lambda v: ((P1(v)[:, 0] + P1(v)[:, 1]) + P1(v)[:, 2])
                        tocc, mocc = T(P3, delta, ey, ex)
                        po[:, 1 - d], pom[:, 1 - d] = np.where(m, tocc, 1.0), np.where(m, mocc, 1.0)
                        g_iw[d] = np.where(m[:, None], k_p * (timg * o64), 0.0)
                        m_iw[d] = np.where(m[:, None], np.abs(k_p * (mimg * o64)), 0.0)
                    else:
                        s = np.sqrt(delta * delta + 1e-6)
                        e = (s[:, 0] + s[:, 1]) + s[:, 2]
                        po[:, 1 - d] = pom[:, 1 - d] = np.where(m, e, 1.0)
                        g_iw[d] = np.where(m[:, None], k_p * ((delta / s) * o64), 0.0)
                        m_iw[d] = np.abs(g_iw[d])
            so = S(oc, D2) if on["smooth_occ"] else None
            pr = 1.0 - oc[:, ::-1].astype(np.float64) if on["prior_occ"] else None
            to = ([k_p * po] if on["pme"] else []) + ([k_so * so[0]] if so else []) + ([k_pr * pr] if pr is not None else [])
            mo = ([np.abs(k_p * pom)] if on["pme"] else []) + ([abs(k_so) * so[1]] if so else []) + ([np.abs(k_pr * pr)] if pr is not None else [])
            g_o, m_o = TG._sum(to, shape2), (TG._sum(mo, shape2), abs(k_so) * so[2] if so else zero2)
            z3 = np.zeros((n, 3, h, w), np.float64)
            grads += [g_f] + ([g_p] if past else []) + [g_o, g_iw[0], g_iw[1]]
            mags += [m_f] + ([m_p] if past else []) + [m_o, (m_iw[0], z3), (m_iw[1], z3)]
        out = [g.astype(F32) for g in grads]
    return (out, mags, grads) if with_mag else out


def lua_grad_ft(table, ref, past, flow_scale=TL.SCALE, o=None):
    """`gradOutputs` per triplet in float64, as tests/table_loss_grad_fields.lua_grad, with
    criterions/SecondOrderSmoothnessCriterion.lua:77-104 (L1 penalty) for the flows where o["smooth_second_order"] and
    criterions/OBGCCriterion.lua:151-300 (L1 penalty, penalty_out = 1, 1-based fp32 target coordinates) for the photometric term where
    o["pme_criterion"] is "OBGCC", accumulated as train.lua:428-468 does.  The forward differences of each warped image are its own
    (lines 194-195 add them onto those of the image before; include/b2f.h).  A map too small for the slices of
    SecondOrderSmoothnessCriterion (h < 3 or w < 3) has empty slices on that axis."""
    o = o or DEFAULTS
    if not o["smooth_second_order"] and o["pme_criterion"] != "OBGCC":
        return TG.lua_grad(table, ref, past, flow_scale, first_order(o))
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    eps = 0.001 * 0.001
    l1 = lambda x: np.power(x * x + eps, 0.5)
    l1_der = lambda x: x / np.power(x * x + eps, 0.5)
    down = TL.ref_pyramid(ref, L)
    avg = o["size_average"]
    alpha, beta, gamma = o["pme_alpha"], o["pme_beta"], o["pme_gamma"]
    # everything but the two replaced criteria: the first-order transcription with those two weights at 0
    base = dict(first_order(o))
    if o["smooth_second_order"]:
        base["smooth_flow"] = 0.0
    if o["pme_criterion"] == "OBGCC":
        base["pme"] = 0.0
    out = TG.lua_grad(table, ref, past, flow_scale, base)

    def second_order_back(inp, target):
        inp, target = inp.astype(np.float64), target.astype(np.float64)
        gy, gx = np.zeros_like(inp), np.zeros_like(inp)
        gy[:, :, 1:-1, :] = 2 * inp[:, :, 1:-1, :] - inp[:, :, :-2, :] - inp[:, :, 2:, :]
        gx[:, :, :, 1:-1] = 2 * inp[:, :, :, 1:-1] - inp[:, :, :, :-2] - inp[:, :, :, 2:]
        igy = np.zeros((inp.shape[0], 1) + inp.shape[2:])
        igx = np.zeros((inp.shape[0], 1) + inp.shape[2:])
        igy[:, :, 1:, :] += np.mean(np.abs(target[:, :, 1:, :] - target[:, :, :-1, :]), axis=1, keepdims=True)
        igx[:, :, :, 1:] += np.mean(np.abs(target[:, :, :, 1:] - target[:, :, :, :-1]), axis=1, keepdims=True)
        igy[:, :, 1:-1, :] += np.mean(np.abs(target[:, :, 1:-1, :] - target[:, :, 2:, :]), axis=1, keepdims=True)
        igx[:, :, :, 1:-1] += np.mean(np.abs(target[:, :, :, 1:-1] - target[:, :, :, 2:]), axis=1, keepdims=True)
        wy, wx = np.exp(-20.0 * igy), np.exp(-20.0 * igx)
        gy, gx = l1_der(gy) * wy, l1_der(gx) * wx
        g = np.zeros_like(inp)
        g[:, :, 1:-1, :] += 2 * gy[:, :, 1:-1, :]
        g[:, :, :, 1:-1] += 2 * gx[:, :, :, 1:-1]
        g[:, :, :-2, :] += -gy[:, :, 1:-1, :]
        g[:, :, :, :-2] += -gx[:, :, :, 1:-1]
        g[:, :, 2:, :] += -gy[:, :, 1:-1, :]
        g[:, :, :, 2:] += -gx[:, :, :, 1:-1]
        return (1.0 / inp.size) * g if avg else g

    def obgcc_back(sub, target, scaling):
        warp_start = 3 if past else 2          # 0-based index of the first warped image
        occ = sub[warp_start - 1].astype(np.float64)
        target = target.astype(np.float64)
        _, _, h, w = sub[0].shape
        norm = 3.0 / (3.0 * h * w)
        cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
        cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
        target_gy, target_gx = np.zeros_like(target), np.zeros_like(target)
        target_gy[:, :, :-1, :] = target[:, :, 1:, :] - target[:, :, :-1, :]
        target_gx[:, :, :, :-1] = target[:, :, :, 1:] - target[:, :, :, :-1]
        g_occ = np.zeros_like(occ)
        g_img = []
        for f in (1, 2):
            img = sub[warp_start - 1 + f].astype(np.float64)
            img_gy, img_gx = np.zeros_like(img), np.zeros_like(img)
            img_gy[:, :, :-1, :] = img[:, :, 1:, :] - img[:, :, :-1, :]
            img_gx[:, :, :, :-1] = img[:, :, :, 1:] - img[:, :, :, :-1]
            buf = img - target
            gi = l1_der(buf) * alpha
            buf_gy = img_gy - target_gy
            gi = gi + -1 * (l1_der(buf_gy) * gamma)
            gi[:, :, 1:, :] += l1_der(buf_gy[:, :, :-1, :]) * gamma
            buf_gx = img_gx - target_gx
            gi = gi + -1 * (l1_der(buf_gx) * beta)
            gi[:, :, :, 1:] += l1_der(buf_gx[:, :, :, :-1]) * beta
            buf = l1(buf).sum(axis=1) * alpha
            buf = buf + -1 * (l1(buf_gy).sum(axis=1) * gamma)
            buf[:, 1:, :] += l1(buf_gy[:, :, :-1, :]).sum(axis=1) * gamma
            buf = buf + -1 * (l1(buf_gx).sum(axis=1) * beta)
            buf[:, :, 1:] += l1(buf_gx[:, :, :, :-1]).sum(axis=1) * beta
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

    with np.errstate(all="ignore"):
        for b in range(n):
            for l in range(L):
                sub = [t[b:b + 1] for t in table[l * per:(l + 1) * per]]
                dst = [g[b:b + 1] for g in out[l * per:(l + 1) * per]]
                target = down[l][b:b + 1]
                lw = o["level_weights"][l]
                if o["smooth_second_order"]:
                    for i in range(2 if past else 1):
                        dst[i] += lw * o["smooth_flow"] * second_order_back(sub[i], target)
                if o["pme_criterion"] == "OBGCC":
                    for i, v in enumerate(obgcc_back(sub, target, flow_scale / 2.0 ** l)):
                        dst[per - 3 + i] += lw * o["pme"] * v
    return out


def torch_terms(tensors, ref, past, flow_scale=TL.SCALE, o=None, inside=None):
    """the two fine-tuning criteria of train.lua:428-468 as one torch float64 scalar, summed over the triplets (each a batch of one): the
    forward values of SecondOrderSmoothnessCriterion.lua:28-75 on the flows and of OBGCCriterion.lua:39-149 on `tensors` (torch float64,
    the table), both with the L1 penalty, beta and gamma as updateOutput applies them and the brightness part times alpha, which
    updateOutput leaves out (quirk 1; the tests that use this take alpha = 1).  The contrast weights and the inside masks are constants."""
    import torch
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(tensors) // per
    avg = o["size_average"]
    down = TL.ref_pyramid(ref, L)
    total = 0.0
    l1 = lambda x: torch.sqrt(x * x + 1e-6)
    for l in range(L):
        sub = tensors[l * per:(l + 1) * per]
        R = torch.from_numpy(down[l].astype(np.float64))
        n, _, h, w = R.shape
        lw = o["level_weights"][l]
        if o["smooth_second_order"] and o["smooth_flow"] != 0.0:
            igx, igy = torch.zeros(n, 1, h, w, dtype=torch.float64), torch.zeros(n, 1, h, w, dtype=torch.float64)
            igy[:, :, 1:, :] += (R[:, :, 1:, :] - R[:, :, :-1, :]).abs().mean(dim=1, keepdim=True)
            igx[:, :, :, 1:] += (R[:, :, :, 1:] - R[:, :, :, :-1]).abs().mean(dim=1, keepdim=True)
            igy[:, :, 1:-1, :] += (R[:, :, 1:-1, :] - R[:, :, 2:, :]).abs().mean(dim=1, keepdim=True)
            igx[:, :, :, 1:-1] += (R[:, :, :, 1:-1] - R[:, :, :, 2:]).abs().mean(dim=1, keepdim=True)
            wy, wx = torch.exp(-20.0 * igy), torch.exp(-20.0 * igx)
            for i in range(2 if past else 1):
                F = sub[i]
                gy = 2 * F[:, :, 1:-1, :] - F[:, :, :-2, :] - F[:, :, 2:, :]
                gx = 2 * F[:, :, :, 1:-1] - F[:, :, :, :-2] - F[:, :, :, 2:]
                s = (l1(gy) * wy[:, :, 1:-1, :]).sum() + (l1(gx) * wx[:, :, :, 1:-1]).sum()   # (the border adds the constant P1(0) * w)
                total = total + lw * o["smooth_flow"] * (s / (2.0 * h * w) if avg else s)
        if o["pme_criterion"] == "OBGCC" and o["pme"] != 0.0:
            occ = sub[per - 3]
            kd = float(F32(flow_scale / 2.0 ** l))
            acc = 0.0
            for d in range(2):
                fl = sub[1] if (d == 0 and past) else sub[0]
                _, _, nan, ins = FW.coordinates(fl.detach().numpy().astype(F32), -kd if d == 0 else kd)
                m = torch.from_numpy((ins & ~nan).astype(np.float64))
                I = sub[per - 2 + d]
                ex = (I[:, :, :, 1:] - I[:, :, :, :-1]) - (R[:, :, :, 1:] - R[:, :, :, :-1])
                ey = (I[:, :, 1:, :] - I[:, :, :-1, :]) - (R[:, :, 1:, :] - R[:, :, :-1, :])
                e = o["pme_alpha"] * l1(I - R).sum(dim=1)
                e = e + o["pme_beta"] * torch.nn.functional.pad(l1(ex).sum(dim=1), (0, 1))      # (the last column adds the constant P1(0))
                e = e + o["pme_gamma"] * torch.nn.functional.pad(l1(ey).sum(dim=1), (0, 0, 0, 1))
                e = e * occ[:, 1 - d]
                acc = acc + (e * m + (1.0 - m)).sum()
            acc = acc / 6.0
            total = total + lw * o["pme"] * (acc / (h * w) if avg else acc)
    return total
