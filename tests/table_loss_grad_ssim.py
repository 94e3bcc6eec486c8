"""Shared by tests/test_table_loss_grad_ssim_cpu.py and tests/test_gpu_table_loss_grad_ssim.py: `want_grad_ssim`, the plain numpy
restatement of include/b2f.h's definition of the gradient table with the occlusion-aware SSIM + L1 photometric term (the *_grad_ssim
entries) that the host entry is held against bit for bit, and `lua_grad_ssim`, a float64 transcription of
OSSIML1Criterion:updateGradInput (criterions/OSSIML1Criterion.lua:165-302) beside the other criteria, accumulated as train.lua:428-468
does, that shares nothing with the restatement's photometric part (a 2-D kernel from the Gaussian formula, torch's replicate padding
and conv2d).  Everything the definition takes over from the *_grad_ft entries -- the flow planes, S(o, D2), the coefficients -- comes
from tests/table_loss_grad_ft_fields.py; the ranges and the window from tests/table_loss_ssim_fields.py."""
import numpy as np

from back2future_amd import back2future
from tests import flow_warp_fields as FW
from tests import table_loss_fields as TL
from tests import table_loss_grad_fields as TG
from tests import table_loss_grad_ft_fields as TF
from tests import table_loss_ssim_fields as TS

F32 = np.float32
TERMS = TG.TERMS
BATCH, IMAGE, GIVEN = TS.BATCH, TS.IMAGE, TS.GIVEN
DEFAULTS = dict(TG.DEFAULTS, smooth_second_order=False, ssim_alpha=0.85)
# wrong readings of the definition that the bit-for-bit tests must tell from the right one
MUTATIONS = ("border_weight", "span_factor", "other_occlusion", "l_dcs_dropped", "zero_padding")


def options(**kw):
    """the options as a dict: DEFAULTS with the keywords replaced"""
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def struct(o):
    """the dict as the b2f_loss_grad_ssim_opts the entries take"""
    wt = dict((k, o[k]) for k in TERMS)
    wt["level_weights"] = o["level_weights"]
    return back2future.loss_grad_ssim_options(weights=wt, size_average=o["size_average"], smooth_second_order=o["smooth_second_order"],
                                              ssim_alpha=o["ssim_alpha"])


def ft_options(o, **kw):
    """the options of tests/table_loss_grad_ft_fields.py that share every term but the photometric one (OBCC there)"""
    r = TF.options(pme_criterion="OBCC", pme_alpha=1.0, pme_beta=1.0, pme_gamma=1.0, smooth_second_order=bool(o["smooth_second_order"]))
    r.update(dict((k, o[k]) for k in TERMS + ("level_weights", "size_average")))
    r.update(kw)
    return r


def range_arg(mode, ranges):
    """the keyword ssim_range of the Python entry points for (mode, ranges)"""
    return "batch" if mode == BATCH else "image" if mode == IMAGE else np.asarray(ranges, F32)


def used_ranges(R, iw, mode, ranges, j, L):
    """(mn, mx) as float64 arrays (n, 1, 1, 1): the range of every image at level j (include/b2f.h, the *_ssim entries)"""
    n = R.shape[0]
    if mode == BATCH:
        used = [TS.own_range_bits([R, iw[0], iw[1]])] * n
    elif mode == IMAGE:
        used = [TS.own_range_bits([R[b], iw[0][b], iw[1][b]]) for b in range(n)]
    else:
        g = np.asarray(ranges, F32).reshape(L, 2)[j].view(np.uint32)
        used = [(g[0], g[1])] * n
    mn = np.array([TS._as_float(u[0]) for u in used], np.float64).reshape(n, 1, 1, 1)
    mx = np.array([TS._as_float(u[1]) for u in used], np.float64).reshape(n, 1, 1, 1)
    return mn, mx


def want_grad_ssim(table, ref, past, flow_scale=TL.SCALE, o=None, mode=BATCH, ranges=None, mutation=None, with_mag=False):
    """the gradient table (float32 arrays with the table's shapes) by include/b2f.h's definition: fp64, one rounding to fp32.
    mutation: one of MUTATIONS.  with_mag: also, per tensor, the sum of the magnitudes of the fp64 terms of every element with l and
    cs counted as 1 and every difference as the sum of its operands' magnitudes (what the bar of lua_grad_ssim scales with; the flow
    planes: None, they are those of want_grad_ft), and the fp64 sums before the rounding"""
    assert mutation is None or mutation in MUTATIONS
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    pyr = TL.ref_pyramid(ref, L)
    ge, gc = TS.weights()
    zp = mutation == "zero_padding"
    alpha = float(o["ssim_alpha"])
    beta = 1.0 - alpha
    D1 = lambda v: v / np.sqrt(v * v + 1e-6)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    G = lambda a: TS._window(a, ge, gc, zp)
    # the flow planes do not read the photometric term; S(o, D2) is the only term of the occlusion planes with every other weight 0
    flows, _, flows64 = TF.want_grad_ft(table, ref, past, flow_scale, ft_options(o, pme=0.0), with_mag=True)
    on = dict((k, o[k] != 0.0) for k in TERMS)
    so64 = None
    if on["smooth_occ"]:
        so64 = TF.want_grad_ft(table, ref, past, flow_scale, ft_options(o, smooth_flow=0.0, const_vel=0.0, pme=0.0, prior_occ=0.0), with_mag=True)[2]
    grads, mags = [], []
    with np.errstate(all="ignore"):
        for j in range(L):
            t = table[j * per:(j + 1) * per]
            f, p, oc, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
            R = pyr[j]
            n, _, h, w = R.shape
            _, _, k_p, k_so, k_pr = TG.coefficients(o, j, h, w)
            shape2 = (n, 2, h, w)
            po, pom = np.zeros(shape2, np.float64), np.zeros(shape2, np.float64)
            g_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            m_iw = [np.zeros((n, 3, h, w), np.float64), np.zeros((n, 3, h, w), np.float64)]
            if on["pme"]:
                kd = float(F32(flow_scale / 2.0 ** j))
                mn, mx = used_ranges(R, iw, mode, ranges, j, L)
                norm = lambda a: (a.astype(np.float64) - mn) / (mx - mn)
                y = norm(R)
                mu_y = G(y)
                gyy = G(y * y)
                gw = gc * gc
                if mutation == "border_weight":     # the weight the pixel really has in its own window under replication
                    cx = gc + ge * (np.arange(w) == 0) + ge * (np.arange(w) == w - 1)
                    cy = gc + ge * (np.arange(h) == 0) + ge * (np.arange(h) == h - 1)
                    gw = cy[:, None] * cx[None, :]
                for d in range(2):
                    fl = p if (d == 0 and past) else f
                    _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
                    m = inside & ~nan
                    o64 = oc[:, (d if mutation == "other_occlusion" else 1 - d)].astype(np.float64)[:, None]
                    x = norm(iw[d])
                    mu_x = G(x)
                    gxx, gxy = G(x * x), G(x * y)
                    xx, yy, xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
                    s_x, s_y, s_xy = gxx - xx, gyy - yy, gxy - xy
                    A, Bd = (xx + yy) + 1e-4, (s_x + s_y) + 9e-4
                    l, cs = (2.0 * xy + 1e-4) / A, (2.0 * s_xy + 9e-4) / Bd
                    dl = ((2.0 * gw) * (mu_y - mu_x * l)) / A
                    dcs = ((2.0 * gw) * ((y - mu_y) - cs * (x - mu_x))) / Bd
                    Q = dl * cs if mutation == "l_dcs_dropped" else dl * cs + l * dcs
                    mQ = np.abs((2.0 * gw) * (np.abs(mu_y) + np.abs(mu_x)) / A) + np.abs((2.0 * gw) * ((np.abs(y) + np.abs(mu_y)) + (np.abs(x) + np.abs(mu_x))) / Bd)
                    terms, tm = [], []
                    if alpha != 0.0:
                        terms.append(-(alpha * Q))
                        tm.append(alpha * mQ)
                    if beta != 0.0:
                        terms.append(beta * D1(x - y))
                        tm.append(np.abs(beta * D1(x - y)))
                    T, Tm = TG._sum(terms, x.shape), TG._sum(tm, x.shape)
                    if mutation == "span_factor":
                        T = T / (mx - mn)
                    g_iw[d] = np.where(m[:, None], k_p * (T * o64), 0.0)
                    m_iw[d] = np.where(m[:, None], np.abs(k_p * (Tm * np.abs(o64))), 0.0)
                    one, e = 1.0 - l * cs, P1(x - y)
                    S, B = (one[:, 0] + one[:, 1]) + one[:, 2], (e[:, 0] + e[:, 1]) + e[:, 2]
                    pt = ([alpha * S] if alpha != 0.0 else []) + ([beta * B] if beta != 0.0 else [])
                    ptm = ([alpha * 6.0 * np.ones_like(S)] if alpha != 0.0 else []) + ([np.abs(beta * B)] if beta != 0.0 else [])
                    po[:, 1 - d] = np.where(m, TG._sum(pt, S.shape), 1.0)
                    pom[:, 1 - d] = np.where(m, TG._sum(ptm, S.shape), 1.0)
            pr = 1.0 - oc[:, ::-1].astype(np.float64) if on["prior_occ"] else None
            so = so64[j * per + per - 3] if on["smooth_occ"] else None
            to = ([k_p * po] if on["pme"] else []) + ([so] if so is not None else []) + ([k_pr * pr] if pr is not None else [])
            mo = ([np.abs(k_p * pom)] if on["pme"] else []) + ([np.abs(so)] if so is not None else []) + ([np.abs(k_pr * pr)] if pr is not None else [])
            g_o, m_o = TG._sum(to, shape2), TG._sum(mo, shape2)
            grads += [flows64[j * per]] + ([flows64[j * per + 1]] if past else []) + [g_o, g_iw[0], g_iw[1]]
            mags += [None] + ([None] if past else []) + [m_o, m_iw[0], m_iw[1]]
        out = [g.astype(F32) for g in grads]
    for j in range(L):      # the flow planes: want_grad_ft's own rounding
        for i in range(2 if past else 1):
            out[j * per + i] = flows[j * per + i]
    return (out, mags, grads) if with_mag else out


def ossiml1_back(sub, target, past, scaling, alpha, mn, mx, size_average, masked=True):
    """OSSIML1Criterion:updateGradInput on one triplet (lines 165-302) in torch float64, line by line -> [g_occ, g_img1, g_img2] as
    numpy arrays; mn, mx: the range updateOutput left in self.mn / self.mx; masked=False: gradCheck's branch (no out-of-image mask)"""
    import torch
    import torch.nn.functional as F
    kernel = torch.from_numpy(TS.gaussian3())
    weight = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
    for c in range(3):
        weight[c, c] = kernel                                                      # lines 38-44
    conv = lambda a: F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), weight)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    warp_start = 3 if past else 2          # 0-based index of the first warped image
    _, _, h, w = sub[0].shape
    norm = 3.0 / (3.0 * h * w)                                                     # line 179
    y = (T(target) - mn) / (mx - mn)                                               # self.target, line 72
    mu_y = conv(y)                                                                 # lines 97-98
    sigma_y = conv(y ** 2) - mu_y ** 2
    occ = T(sub[warp_start - 1])
    cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
    cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
    g_occ = torch.zeros_like(occ)                                                  # line 193
    g_img = []
    for f in (1, 2):
        img = (T(sub[warp_start - 1 + f]) - mn) / (mx - mn)                        # line 197
        buffer = img - y                                                           # line 202
        mu_x = conv(img)                                                           # lines 207-209
        sigma_x = conv(img ** 2) - mu_x ** 2
        sigma_xy = conv(img * y) - mu_x * mu_y
        ssim_l = (2 * mu_x * mu_y + TS.C1) / (mu_x ** 2 + mu_y ** 2 + TS.C1)       # lines 212-213
        ssim_cs = (2 * sigma_xy + TS.C2) / (sigma_x + sigma_y + TS.C2)
        gw = kernel[1, 1]                                                          # line 216
        d_l = 2 * gw * ((mu_y - mu_x * ssim_l) / (mu_x ** 2 + mu_y ** 2 + TS.C1))  # line 217
        d_cs = 2 * gw * (((y - mu_y) - ssim_cs * (img - mu_x)) / (sigma_x + sigma_y + TS.C2))   # line 218
        gi = -alpha * (d_l * ssim_cs + ssim_l * d_cs) + (1 - alpha) * (buffer / torch.sqrt(buffer * buffer + 0.001 * 0.001))   # line 222
        buf = alpha * (1 - ssim_l * ssim_cs).sum(1) + (1 - alpha) * torch.sqrt(buffer * buffer + 0.001 * 0.001).sum(1)        # line 224
        if f <= 1.0:
            fl = sub[1] if past else sub[0]
            tx = cx + (F32(f - 1 - 1) * fl[:, 0]) * F32(scaling)
            ty = cy + (F32(f - 1 - 1) * fl[:, 1]) * F32(scaling)
            ch = 1
        else:
            tx = cx + (F32(f - 1) * sub[0][:, 0]) * F32(scaling)
            ty = cy + (F32(f - 1) * sub[0][:, 1]) * F32(scaling)
            ch = 0
        if masked:
            mask = torch.from_numpy(((tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)).astype(np.float64))
            buf = buf * mask + (1.0 - mask) * 1.0                                  # lines 243-245, 271-273
            gi = gi * mask[:, None]                                                # lines 249, 277
        g_occ[:, ch] += buf                                                        # lines 253, 281
        gi = gi * occ[:, ch][:, None]                                              # lines 257, 285
        gi = gi * (1.0 / (3 * 2))                                                  # line 289
        g_img.append((gi * norm if size_average else gi).numpy())
    g_occ = g_occ * (1.0 / (3 * 2))                                                # line 296
    return [(g_occ * norm if size_average else g_occ).numpy()] + g_img


def lua_grad_ssim(table, ref, past, flow_scale=TL.SCALE, o=None, ranges=None):
    """`gradOutputs` per triplet in float64: tests/table_loss_grad_ft_fields.lua_grad_ft for every criterion but the photometric one,
    and OSSIML1Criterion:updateGradInput (`ossiml1_back`) with the range of the whole batch (lines 62-67: what the reference computes
    when the n triplets are one batch) or, with ranges (L x 2), the given one; accumulated as train.lua:428-468 does"""
    o = o or DEFAULTS
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    out = TF.lua_grad_ft(table, ref, past, flow_scale, ft_options(o, pme=0.0))
    down = TL.ref_pyramid(ref, L)
    with np.errstate(all="ignore"):
        for l in range(L):
            lv = table[l * per:(l + 1) * per]
            if ranges is None:
                vals = [down[l], lv[per - 2], lv[per - 1]]
                mn, mx = float(min(float(v.min()) for v in vals)), float(max(float(v.max()) for v in vals))
            else:
                mn, mx = float(F32(ranges[l][0])), float(F32(ranges[l][1]))
            for b in range(n):
                sub = [t[b:b + 1] for t in lv]
                dst = [g[b:b + 1] for g in out[l * per:(l + 1) * per]]
                back = ossiml1_back(sub, down[l][b:b + 1], past, flow_scale / 2.0 ** l, o["ssim_alpha"], mn, mx, o["size_average"])
                for i, v in enumerate(back):
                    dst[per - 3 + i] += o["level_weights"][l] * o["pme"] * v
    return out


def allowance_ssim_grad():
    """`a` of the bar 2^-24 |v| + 2^-149 + a m between want_grad_ssim and lua_grad_ssim, derived and not measured.  Both evaluate the same
    expressions in float64; they differ by the window's association (the separable sums against conv2d's nine products) and by how the
    quotients are grouped.  eps = 2^-53, every normalised value in [0, 1] (the batch range holds the values).  From
    tests/table_loss_ssim_fields.allowance_ssim: a window sum is within 20 eps, a product of two within 41 eps, a sigma within 62 eps; all
    window sums and means are >= 0, so l, a quotient of sums of non-negative numbers, is within 200 eps *relatively*; cs = N / Bd with
    Bd >= C2 is within 251 eps / C2 absolutely, and the relative error of Bd is within 126 eps / C2, of A within 84 eps / (A) <= 168 eps
    relatively (A is a sum of non-negative numbers: twice the products' 41 eps relative, and the roundings).  m counts l and cs as 1 and
    every difference as the sum of its operands' magnitudes, so that each error below is a multiple of a summand of m:
      dl  = 2 gw (mu_y - mu_x l) / A:   numerator within (20 + 20 + 200 + 2) eps of (mu_y + mu_x); the division by A adds 168 eps + eps:
            within 411 eps of its summand 2 gw (mu_y + mu_x) / A
      dcs = 2 gw ((y - mu_y) - cs (x - mu_x)) / Bd:   the numerator within 22 eps (y + mu_y) + (251 eps / C2 + 22 eps)(x + mu_x); the
            division by Bd adds 126 eps / C2 relatively: within (251 + 126) eps / C2 + 50 eps of its summand -- the division by Bd >= C2
            enters twice, once through cs and once directly
      Q = dl cs + l dcs:   dl (counted with cs as 1) times the error of cs, 251 eps / C2, and its own; l dcs with l's 200 eps:
            within (411 + 251 / C2) eps of dl's summand plus ((377 / C2) + 252) eps of dcs's
      the L1 part D1(x - y): x - y is exact up to the normalisation's roundings, which both sides share: within 8 eps of |D1| <= 1
      PO = alpha S + (1 - alpha) B: S is counted as 6 alpha in m (|1 - l cs| <= 2 per channel), its error 3 (200 + 251 / C2 + 2) eps
    The two sides may lie that far on either side of the exact value: twice the largest relative factor, (411 + 251 / C2 + 377 / C2 + 252)
    eps, rounded up."""
    eps = 2.0 ** -53
    return 2.0 * (411.0 + 251.0 / TS.C2 + 377.0 / TS.C2 + 252.0) * eps
