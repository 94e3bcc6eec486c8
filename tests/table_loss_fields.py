"""Shared by tests/test_table_loss_cpu.py and tests/test_gpu_table_loss.py: the synthetic output tables the unsupervised validation
loss (test.lua:266-297) is tested on, `want`, the plain numpy restatement of include/b2f.h's definition of the record that the host
entry is held against, and `lua_loss`, a float64 transcription of the reference's five criteria and of the loop of test.lua:266-297."""
import numpy as np

from oracle import oracle
from tests import flow_warp_fields as FW

WORDS = 16
PIXELS, SMOOTH_FLOW, SMOOTH_PAST, CONST_VEL, SMOOTH_OCC, PRIOR_OCC, INSIDE, OUTSIDE, OCHARB, PHOTO_NONFINITE, NONFINITE = 0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14
SCALE = 20.0
F32 = np.float32
LEVEL_WEIGHTS = (0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28)   # test.lua:29-31
WEIGHTS = {"smooth_flow": 1.0, "const_vel": 1.0, "pme": 1.0, "smooth_occ": 0.1, "prior_occ": 0.1}   # opts.lua:61-73


def reference_image(n, H, W, seed=0, tame=False):
    """n x 3 x H x W float32: the left quarter flat (contrast weight exactly 1 on every level), the next quarter a ramp in x and y
    (0.01 and 0.02 per pixel: the weights down its rows are strictly between 0 and 1, e^-0.4 .. e^-6.4 over five levels), the right
    half blocks of sixteen columns (one pixel of the fifth level) at -2.4 / +2.4 in every channel (hard edges: weight about e^-96) and, unless tame, one NaN in image 0."""
    r = np.random.default_rng(seed * 104729 + H * 1000 + W)
    ys, xs = np.arange(H, dtype=F32)[:, None], np.arange(W, dtype=F32)[None, :]
    ref = np.empty((n, 3, H, W), F32)
    for b in range(n):
        for c in range(3):
            flat = np.full((H, W), F32(r.uniform(-2.0, 2.0)), F32)   # (|warped - R| stays below 16 / 3: no saturated photo term)
            ramp = (F32(0.01) * xs + F32(0.02) * ys + F32(0.1 * c)).astype(F32)
            edge = np.where((np.arange(W) // 16) % 2 == 0, F32(-2.4), F32(2.4))[None, :].repeat(H, 0).astype(F32)
            col = np.arange(W)[None, :].repeat(H, 0)
            ref[b, c] = np.where(col < W // 4, flat, np.where(col < W // 2, ramp, edge))
    if not tame and H * W >= 64:
        ref[0, 1, H // 2 + 1, W // 8] = np.nan
    return ref


def tables(H, W, L, past, n=2, seed=0, tame=False):
    """(table, ref): the L x (5 if past else 4) tensors of an output table in table order -- per level j, at (H >> j) x (W >> j): the
    future flow, the past flow (past), the occlusions, warped image 1, warped image 3 -- and the reference image n x 3 x H x W.  The
    flows are those of flow_warp_fields.fields at the level's size times 2^j, so that they meet the level's scale 20 / 2^j as that
    module's flows meet 20 (whole pixels, zeros, targets off every side and exactly on the border, NaN and +-Inf); the occlusions
    carry exact 0, 0.5 and 1 and a NaN.  tame: every non-finite value replaced (flows by 0, probabilities by 0.25) and the flows
    left at that module's magnitudes on every level and clipped to +-3 (60 pixels at scale 20: the band still leaves images of up to
    96 pixels on every side), so that no pixel term reaches the record's saturation at 16 (N(0, 0.6) times 2^4 would, and so would the
    corners of a band of +-5): the fields loss_summary is held against lua_loss on, which knows no saturation."""
    table = []
    for j in range(L):
        h, w = H >> j, W >> j
        flow, ims, prob = FW.fields(h, w, n=n, seed=seed + 10 * j)
        flow_p, ims_p, _ = FW.fields(h, w, n=n, seed=seed + 10 * j + 5)
        fl = [flow * F32(1 if tame else 2 ** j), flow_p * F32(1 if tame else 2 ** j)]
        if tame:
            fl = [np.clip(np.where(np.isfinite(f), f, F32(0)), F32(-3), F32(3)).astype(F32) for f in fl]
            prob = np.where(np.isfinite(prob), prob, F32(0.25)).astype(F32)
        # warped images: the byte images of the fields moved into the value range of normalized frames
        iw1 = ((ims[0] - F32(0.45)) / F32(0.225)).astype(F32)
        iw3 = ((ims_p[2] - F32(0.45)) / F32(0.225)).astype(F32)
        table += [fl[0]] + ([fl[1]] if past else []) + [prob, iw1, iw3]
    return [np.ascontiguousarray(t, F32) for t in table], reference_image(n, H, W, seed, tame)


def ref_pyramid(ref, L):
    """R_0 .. R_{L-1}: R_j = nn.SpatialAveragePooling(2,2,2,2) of R_{j-1} in fp32 (oracle.avgpool2; test.lua:132,269)"""
    out = [np.ascontiguousarray(ref, F32)]
    for _ in range(1, L):
        out.append(oracle.avgpool2(out[-1]))
    return out


_C = [1.0]
for _i in range(1, 14):
    _C.append(_C[-1] / _i)


def E(t):
    """include/b2f.h's exponential for t <= 0 in float64 numpy, operation by operation"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        tt = np.where(t > 0.0, 0.0, t)
        k = np.rint(tt * 1.44269504088896338700e+00)
        r = (tt - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
        p = np.full_like(r, _C[13])
        for i in range(12, -1, -1):
            p = p * r + _C[i]
        out = np.ldexp(p, np.where(np.isfinite(k), k, 0.0).astype(np.int64))
        out = np.where(tt < -708.0, 0.0, out)
    return np.where(np.isnan(t), t, out)


def _diffs(a):
    """forward differences of n x C x h x w in float64: (dx, dy), zero in the last column / row"""
    a = a.astype(np.float64)
    dx, dy = np.zeros_like(a), np.zeros_like(a)
    with np.errstate(all="ignore"):
        dx[..., :, :-1] = a[..., :, 1:] - a[..., :, :-1]
        dy[..., :-1, :] = a[..., 1:, :] - a[..., :-1, :]
    return dx, dy


def _q30_sum(t, mask=None):
    """per image: the sum of q30 over the pixels whose term is no NaN (and in mask)"""
    ok = ~np.isnan(t) if mask is None else (~np.isnan(t) & mask)
    q = FW.q30(np.where(ok, t, 0.0))
    return np.array([q[b][ok[b]].sum(dtype=np.uint64) for b in range(t.shape[0])], np.uint64)


def want(table, ref, past, flow_scale=SCALE):
    """uint64 (n, L, 16): the definition of include/b2f.h, one expression per word"""
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    pyr = ref_pyramid(ref, L)
    rec = np.zeros((n, L, WORDS), np.uint64)
    P1 = lambda v: np.sqrt(v * v + 1e-6)
    P2 = lambda v: v * v
    for j in range(L):
        t = table[j * per:(j + 1) * per]
        f, p, o, iw = t[0], (t[1] if past else None), t[per - 3], (t[per - 2], t[per - 1])
        R = pyr[j]
        h, w = R.shape[2:]
        with np.errstate(all="ignore"):
            rdx, rdy = _diffs(R)
            wx = E(-20.0 * ((np.abs(rdx[:, 0]) + np.abs(rdx[:, 1])) + np.abs(rdx[:, 2])) / 3.0)
            wy = E(-20.0 * ((np.abs(rdy[:, 0]) + np.abs(rdy[:, 1])) + np.abs(rdy[:, 2])) / 3.0)

            def smooth(a, pen):
                dx, dy = _diffs(a)
                return (pen(dx[:, 0]) * wx + pen(dy[:, 0]) * wy) + (pen(dx[:, 1]) * wx + pen(dy[:, 1]) * wy)

            terms = {SMOOTH_FLOW: smooth(f, P1), SMOOTH_OCC: smooth(o, P2),
                     PRIOR_OCC: 1.0 - o[:, 0].astype(np.float64) * o[:, 1].astype(np.float64)}
            if past:
                terms[SMOOTH_PAST] = smooth(p, P1)
                d = f.astype(np.float64) - p.astype(np.float64)
                terms[CONST_VEL] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        bad = np.zeros((n, h, w), bool)
        for word, term in terms.items():
            rec[:, j, word] = _q30_sum(term)
            bad |= np.isnan(term)
        rec[:, j, PIXELS] = h * w
        rec[:, j, NONFINITE] = bad.reshape(n, -1).sum(axis=1)
        kd = float(F32(flow_scale / 2.0 ** j))
        for d in range(2):
            fl = p if (d == 0 and past) else f
            _, _, nan, inside = FW.coordinates(fl, -kd if d == 0 else kd)
            with np.errstate(all="ignore"):
                delta = iw[d].astype(np.float64) - R.astype(np.float64)
                s = np.sqrt(delta * delta + 1e-6)
                e = (s[:, 0] + s[:, 1]) + s[:, 2]
                wt = o[:, 1 - d].astype(np.float64)
                we = wt * e
            nonf = nan | (inside & (np.isnan(e) | np.isnan(we) | np.isnan(wt)))
            good = inside & ~nonf
            rec[:, j, INSIDE + d] = good.reshape(n, -1).sum(axis=1)
            rec[:, j, OUTSIDE + d] = (~nan & ~inside).reshape(n, -1).sum(axis=1)
            rec[:, j, OCHARB + d] = _q30_sum(np.where(good, we, 0.0), good)
            rec[:, j, PHOTO_NONFINITE + d] = nonf.reshape(n, -1).sum(axis=1)
    return rec


def inside_masks(flow, k):
    """(0-based fp32 mask of include/b2f.h, 1-based fp32 mask of OBCCriterion.lua:97-100) of the targets of flow * k"""
    n, _, h, w = flow.shape
    _, _, _, zero_based = FW.coordinates(flow, k)
    with np.errstate(all="ignore"):
        tx = np.arange(1, w + 1, dtype=F32)[None, None, :] + flow[:, 0] * F32(k)
        ty = np.arange(1, h + 1, dtype=F32)[None, :, None] + flow[:, 1] * F32(k)
        one_based = (tx >= 1) & (ty >= 1) & (tx <= w) & (ty <= h)
    return zero_based, one_based


def lua_loss(table, ref, past, flow_scale=SCALE, like="test", size_average=False, weights=None):
    """float64 array (n,): the loop of test.lua:266-297 (like="test") or the sum of train.lua:428-432 (like="train") per triplet, the
    five criteria transcribed in float64: criterions/SmoothnessCriterion.lua:28-73 (L1 penalty for flows, quadratic for occlusions,
    model.lua:204-216), ConstVelCriterion.lua:29-46, OBCCriterion.lua:36-119 (L1 penalty, penalty_out = 1, pwc_flow_scaling =
    flow_scale / 2^l as train.lua:425 sets it; target coordinates 1-based fp32 as in flow_warp_fields.obcc_l1),
    OcclusionPriorCriterion.lua:28-49.  Each triplet is a batch of one, so sizeAverage's norms are per triplet."""
    wt = dict(WEIGHTS)
    wt.update(weights or {})
    per = 5 if past else 4
    L = len(table) // per
    n = ref.shape[0]
    n_flow = 2 if past else 1
    eps = 0.001 * 0.001
    l1 = lambda x: np.power(x * x + eps, 0.5)
    quad = lambda x: x * x
    down = ref_pyramid(ref, L)
    out = np.zeros(n, np.float64)

    def smoothness(inp, target, pen):
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

    def const_vel(a, b):
        d = a.astype(np.float64) - b.astype(np.float64)
        o = np.sqrt((d * d).sum(axis=1)).sum()
        return o / a.size if size_average else o

    def obcc(sub, target, scaling):
        warp_start = 3 if past else 2          # 0-based index of the first warped image
        occ = sub[warp_start - 1].astype(np.float64)
        _, _, h, w = sub[0].shape
        cx = np.arange(1, w + 1, dtype=F32)[None, None, :]
        cy = np.arange(1, h + 1, dtype=F32)[None, :, None]
        acc = np.zeros((1, h, w), np.float64)
        for f in (1, 2):
            img = sub[warp_start - 1 + f].astype(np.float64)
            tmp = l1(img - target.astype(np.float64)).sum(axis=1)
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

    for b in range(n):
        err = 0.0
        for l in range(L):
            sub = [t[b:b + 1] for t in table[l * per:(l + 1) * per]]
            target = down[l][b:b + 1]
            lw = LEVEL_WEIGHTS[l]
            if like == "test":
                for _ in range(n_flow):          # test.lua:275-277 passes sub_outs[1] every time
                    err += lw * wt["smooth_flow"] * smoothness(sub[0], target, l1)
            else:
                for i in range(n_flow):          # train.lua:428-432 passes sub_outs[i]
                    err += lw * wt["smooth_flow"] * smoothness(sub[i], target, l1)
            if past:
                err += lw * wt["const_vel"] * const_vel(sub[0], sub[1])
            err += lw * wt["pme"] * obcc(sub, target, flow_scale / 2.0 ** l)
            err += lw * wt["smooth_occ"] * smoothness(sub[per - 3], target, quad)
            err += lw * wt["prior_occ"] * prior(sub[per - 3])
        out[b] = err
    return out


def bound(H, W, L, past, like="test", size_average=False, weights=None, lua=0.0):
    """The bar of loss_summary against lua_loss: each pixel term rounds by at most 2^-31 in the record, so the difference is at most
    the sum over levels and terms of level_weight * weight * (pixel terms) * 2^-31 (times the term's norm with size_average), plus
    1e-12 * |lua_loss| for the float64 sums of the transcription."""
    wt = dict(WEIGHTS)
    wt.update(weights or {})
    n_flow = 2 if past else 1
    total = 0.0
    for j in range(L):
        hw = float((H >> j) * (W >> j))
        half, full = (1.0 / (2.0 * hw), 1.0 / hw) if size_average else (1.0, 1.0)
        t = wt["smooth_flow"] * n_flow * hw * half
        t += (wt["const_vel"] * hw * half) if past else 0.0
        t += wt["pme"] * (2.0 * hw / 6.0) * full
        t += wt["smooth_occ"] * hw * half + wt["prior_occ"] * hw * full
        total += LEVEL_WEIGHTS[j] * t * 2.0 ** -31
    return total + 1e-12 * abs(lua)
