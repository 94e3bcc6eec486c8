"""Shared by tests/test_flow_warp_cpu.py and tests/test_gpu_flow_warp.py: the fields motion compensation is tested on and `want`, the
plain numpy restatement of include/b2f.h's definition (the warp from oracle.warping_unit wherever the flow is finite, the record in
fp64 and Python integers) that the host entry is held against."""
import numpy as np

from oracle import oracle

WORDS = 14
INSIDE, OUTSIDE, CHARB, SQ, OCHARB, WEIGHT, NONFINITE = 0, 2, 4, 6, 8, 10, 12
SCALE = 20.0
F32 = np.float32


def _exact(m, scale=SCALE):
    """raw flow values whose product with `scale` is the whole number m in fp32 (0 where no such value exists)"""
    m = np.asarray(m, F32)
    raw = m / F32(scale)
    return np.where(raw * F32(scale) == m, raw, F32(0)).astype(F32)


def fields(H, W, n=3, kind="unit", seed=0):
    """flow (float32 n x 2 x H x W, raw: pixels / 20), (im1, im2, im3) (n x 3 x H x W, k / 255 as float32 with kind "unit", the bytes k
    with "u8"), occ_prob (float32 n x 2 x H x W).  The flows: N(0, 0.6) raw = +-12 px; every fifth row whole pixels; one row of exact
    zeros; a band of columns whose targets leave the image on each of its four sides; targets exactly on column W - 1 and row H - 1 in
    both directions; a few NaN and +-Inf values.  The probabilities carry exact 0, 0.5 and 1 and, in image 0, a NaN."""
    r = np.random.default_rng(seed * 7919 + H * 1000 + W)
    flow = r.normal(0, 0.6, (n, 2, H, W)).astype(F32)
    ys, xs = np.arange(H), np.arange(W)
    for y in range(0, H, 5):   # whole pixels
        flow[:, :, y] = _exact(np.rint(flow[:, :, y] * F32(SCALE)))
    if H > 2:
        flow[:, :, 2] = 0.0
    if W >= 8 and H >= 8:
        x0, q = W // 2, H // 4
        far = (max(H, W) + 5.0) / SCALE
        flow[:, 0, 0 * q:1 * q, x0:x0 + 2] = -far   # the future target leaves on the left, the past one on the right
        flow[:, 0, 1 * q:2 * q, x0:x0 + 2] = far
        flow[:, 1, 2 * q:3 * q, x0:x0 + 2] = -far   # ... above / below
        flow[:, 1, 3 * q:4 * q, x0:x0 + 2] = far
        # exactly on the last column / row: row 1 for the future frame (k = +20), row 3 for the past one (k = -20)
        flow[:, 0, 1, :] = _exact(W - 1 - xs)
        flow[:, 1, 1, :] = _exact(np.full(W, H - 1 - 1))
        flow[:, 0, 3, :] = -_exact(W - 1 - xs)
        flow[:, 1, 3, :] = -_exact(np.full(W, H - 1 - 3))
        # exactly on column 0 / row 0
        flow[:, 0, 6, :] = _exact(-xs)
        flow[:, 1, 6, :] = _exact(np.full(W, -6))
    specials = [np.nan, np.inf, -np.inf]
    if H * W >= 64:
        for b in range(n):
            for j in range(9):
                i = (j * 37 + 5 * b + 11) % (H * W)
                flow[b, j % 2, i // W, i % W] = specials[j % 3]
    else:   # a tiny image: zero flow, NaN and Inf from image to image
        tiny = [0.0, np.nan, np.inf, -np.inf, 0.01]
        for b in range(n):
            flow[b, 0] = tiny[b % len(tiny)]
            flow[b, 1] = tiny[(b // 2) % len(tiny)] if b else 0.0
    bytes_ = [r.integers(0, 256, (n, 3, H, W), dtype=np.uint8) for _ in range(3)]
    ims = tuple(bytes_) if kind == "u8" else tuple(a.astype(F32) / F32(255) for a in bytes_)
    prob = r.random((n, 2, H, W), dtype=F32)
    pick = r.integers(0, 8, (n, 2, H, W))
    for v, code in ((0.0, 0), (0.5, 1), (1.0, 2)):
        prob[pick == code] = v
    if H * W >= 64:
        prob[0, 0, H // 2, W // 3] = np.nan
        prob[0, 1, H // 3, W // 2] = np.nan
    return flow, ims, prob


def unit(im):
    """frames as the float values the definition uses: bytes are (float)k / 255.0f"""
    return im.astype(F32) / F32(255) if im.dtype == np.uint8 else np.asarray(im, F32)


def quantise(v):
    """image.save's rounding of a float32 array in fp32: v > 0 ? (v < 1 ? floorf(v * 255 + 0.5) : 255) : 0"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        mid = np.floor(np.where((v > 0) & (v < 1), v, F32(0)) * F32(255) + F32(0.5))
        return np.where(v > 0, np.where(v < 1, mid, F32(255)), F32(0)).astype(np.uint8)


def coordinates(flow, k):
    """(xc, yc, nan, inside) of include/b2f.h in fp32: xc = fx * k + (float)x before the clamp"""
    n, _, H, W = flow.shape
    with np.errstate(all="ignore"):
        xc = flow[:, 0] * F32(k) + np.arange(W, dtype=F32)[None, None, :]
        yc = flow[:, 1] * F32(k) + np.arange(H, dtype=F32)[None, :, None]
        nan = np.isnan(xc) | np.isnan(yc)
        inside = (xc >= 0) & (xc <= F32(W - 1)) & (yc >= 0) & (yc <= F32(H - 1))
    return xc, yc, nan, inside


def _numpy_warp(frame, xc, yc):
    """BilinearSamplerBHWD.cu:88-104 in fp32 numpy for coordinates without NaN (the pixels the oracle is not asked about)"""
    n, C, H, W = frame.shape
    with np.errstate(all="ignore"):
        xc = np.minimum(np.maximum(xc, F32(0)), F32(W - 1))
        yc = np.minimum(np.maximum(yc, F32(0)), F32(H - 1))
        xl, yt = np.floor(xc), np.floor(yc)
        xw, yw = F32(1) - (xc - xl), F32(1) - (yc - yt)
    xi, yi = xl.astype(np.int64), yt.astype(np.int64)
    b = np.arange(n)[:, None, None]
    out = np.zeros((n, C, H, W), F32)
    for c in range(C):
        p = frame[:, c]
        tap = lambda dy, dx: np.where((xi + dx <= W - 1) & (yi + dy <= H - 1), p[b, np.minimum(yi + dy, H - 1), np.minimum(xi + dx, W - 1)], F32(0))
        out[:, c] = (xw * yw) * tap(0, 0) + ((F32(1) - xw) * yw) * tap(0, 1) + (xw * (F32(1) - yw)) * tap(1, 0) + \
                    ((F32(1) - xw) * (F32(1) - yw)) * tap(1, 1)
    return out


def q30(t):
    return (np.minimum(np.maximum(t, 0.0), 16.0) * float(1 << 30) + 0.5).astype(np.uint64)


def want(flow, im1, im2, im3, occ_prob=None, flow_scale=SCALE):
    """(warped float32 n x 2 x 3 x H x W, nan bool n x 2 x H x W, photo uint64 n x 14): the definition of include/b2f.h.  The warped
    values are oracle.warping_unit's wherever both flow components are finite, a numpy restatement's where one is +-Inf, 0 where
    the coordinate is NaN; the record is fp64 numpy, one expression per word."""
    n, _, H, W = flow.shape
    frames = (unit(im1), unit(im3))
    ref = unit(im2).astype(np.float64)
    finite = np.isfinite(flow).all(axis=1)
    tame = np.where(finite[:, None], flow, F32(0))
    warped = np.zeros((n, 2, 3, H, W), F32)
    nans = np.zeros((n, 2, H, W), bool)
    photo = np.zeros((n, WORDS), np.uint64)
    for d, k in enumerate((-flow_scale, flow_scale)):
        xc, yc, nan, inside = coordinates(flow, k)
        w = oracle.warping_unit(frames[d], tame, float(F32(k)))
        rest = ~finite & ~nan
        if rest.any():
            alt = _numpy_warp(frames[d], np.where(nan, F32(0), xc), np.where(nan, F32(0), yc))
            w = np.where(rest[:, None], alt, w)
        w = np.where(nan[:, None], F32(0), w).astype(F32)
        warped[:, d], nans[:, d] = w, nan
        with np.errstate(all="ignore"):
            delta = w.astype(np.float64) - ref
            dd = delta * delta
            s = np.sqrt(dd + 1e-6)
            e = (s[:, 0] + s[:, 1]) + s[:, 2]
            sq = (dd[:, 0] + dd[:, 1]) + dd[:, 2]
            if occ_prob is not None:
                wt = occ_prob[:, 1 - d].astype(np.float64)
                we = wt * e
            else:
                wt = we = np.zeros_like(e)
            bad = nan | (~nan & inside & (np.isnan(e) | np.isnan(we) | np.isnan(wt)))
            good = inside & ~bad
            z = lambda t: np.where(good, t, 0.0)
            for b in range(n):
                photo[b, INSIDE + d] = np.count_nonzero(good[b])
                photo[b, OUTSIDE + d] = np.count_nonzero(~nan[b] & ~inside[b])
                photo[b, CHARB + d] = q30(z(e)[b])[good[b]].sum(dtype=np.uint64)
                photo[b, SQ + d] = q30(z(sq)[b])[good[b]].sum(dtype=np.uint64)
                if occ_prob is not None:
                    photo[b, OCHARB + d] = q30(z(we)[b])[good[b]].sum(dtype=np.uint64)
                    photo[b, WEIGHT + d] = q30(z(wt)[b])[good[b]].sum(dtype=np.uint64)
                photo[b, NONFINITE + d] = np.count_nonzero(bad[b])
    return warped, nans, photo


def obcc_l1(flow, im1, im2, im3, occ_prob, flow_scale=SCALE):
    """criterions/OBCCriterion.lua:36-119 transcribed: the L1 penalty (criterions/penalty/L1_function.lua: (x^2 + eps)^0.5 with
    eps = 0.001 * 0.001), penalty_out = 1, sizeAverage, past_flow = false, F = 3, pwc_flow_scaling = flow_scale, on the warps of
    oracle.warping_unit.  The target coordinates are float tensors there (1-based, fp32); everything that is summed is fp64 here."""
    n, _, H, W = flow.shape
    warps = (oracle.warping_unit(unit(im1), flow, float(F32(-flow_scale))), oracle.warping_unit(unit(im3), flow, float(F32(flow_scale))))
    target = unit(im2).astype(np.float64)
    coord_x = np.arange(1, W + 1, dtype=F32)[None, None, :]
    coord_y = np.arange(1, H + 1, dtype=F32)[None, :, None]
    eps = 0.001 * 0.001
    acc = np.zeros((n, H, W), np.float64)
    for f in (1, 2):
        img = warps[f - 1].astype(np.float64)
        buffer = img - target
        tmp = np.power(buffer * buffer + eps, 0.5).sum(axis=1)
        if f <= 1.0:   # ref = 0.5 * (F - 1) = 1
            tx = coord_x + (F32(f - 1 - 1) * flow[:, 0]) * F32(flow_scale)
            ty = coord_y + (F32(f - 1 - 1) * flow[:, 1]) * F32(flow_scale)
            tmp = tmp * occ_prob[:, 1].astype(np.float64)
        else:
            tx = coord_x + (F32(f - 1) * flow[:, 0]) * F32(flow_scale)
            ty = coord_y + (F32(f - 1) * flow[:, 1]) * F32(flow_scale)
            tmp = tmp * occ_prob[:, 0].astype(np.float64)
        mask = ((tx >= 1) & (ty >= 1) & (tx <= W) & (ty <= H)).astype(np.float64)
        tmp = tmp * mask + (1.0 - mask) * 1.0
        acc += tmp
    norm = 3.0 / (n * 3.0 * H * W)
    return norm * (acc.sum() / (3.0 * 2.0))
