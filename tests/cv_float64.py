"""A float64 restatement of the fused bilinear warp + cost volume (warpingUnit x2 + CostVolMulti x2 + JoinTable, pwc.lua:246-267,393-409),
the bar the kernels and the oracle are held to against it, and the flows and shapes of the tests that use it.  Helper, no test.

The sampling position is the operand of the operation, so it is computed as every kernel (and the oracle) computes it: in float32,
float32(x) + float32(k) * flow, clamped to [0, size - 1] FIRST and floored after (getTopLeft of BilinearSamplerBHWD.cu, bhwd_top_left of
csrc/b2f_internal.h).  Everything after the position is float64: wt = 1 - (c - floor c), the four-tap blend with zero weight for a missing
right / bottom neighbour, win x win displacements per direction with d = (qx + n) * win + (qy + n), forward frm[y - qy, x - qx], backward
frm[y + qy, x + qx], out of range 0, divided by C (CostVolMulti.lua:66-100, costvol_cp8_kernel).

Test flows are multiples of 2^-8 with |flow| <= 32 and every k is 5 * 2^-n, so k * flow is exact in float32 and the position is the same
number whether or not a compiler contracts the multiply-add; check_flow asserts it for the flow it is given.

The bar: |got - ref64| <= (C + 16) * 2^-24 * S elementwise and got == 0 where S == 0, with S = (1/C) sum_c |ref_c| * sum_taps w_t |tap_t,c|
the sum of the absolute products.  That is the forward bound of a dot product of C products summed in any order, fused or not
(gamma_C <= C * u up to second order, u = 2^-24), plus at most 16 roundings for the tap weights, the blend (4 products, 3 sums), the division
and the Cp / C fix-up of b2f_op_warp_costvol.  It is derived, not measured."""
import numpy as np

U = 2.0 ** -24


def quantise(flow):
    """the nearest multiple of 2^-8 inside [-32, 32], as float32"""
    return np.clip(np.rint(np.asarray(flow, np.float64) * 256.0) / 256.0, -32.0, 32.0).astype(np.float32)


def check_flow(flow, k):
    f = np.asarray(flow)
    assert f.dtype == np.float32 and f.ndim == 4 and f.shape[1] == 2
    f64 = f.astype(np.float64)
    assert np.array_equal(f64 * 256.0, np.rint(f64 * 256.0)) and np.abs(f64).max() <= 32.0, "flow is not a multiple of 2^-8 within +-32"
    assert np.array_equal((np.float32(k) * f).astype(np.float64), float(np.float32(k)) * f64), "k * flow is not exact in float32"


def _top_left(coord32, size):
    """bhwd_top_left on a float32 coordinate: clamp, then floor; the weight of the top / left tap in float64"""
    assert coord32.dtype == np.float32
    c = np.minimum(np.maximum(coord32, np.float32(0)), np.float32(size - 1))
    fl = np.floor(c)
    return fl.astype(np.int64), 1.0 - (c.astype(np.float64) - fl.astype(np.float64))


def tap_index(flow, k, axis, size):
    """(index of the left / top tap, its weight) of warpingUnit(., flow, k) along axis 0 (x, size w) or 1 (y, size h): B x h x w each"""
    check_flow(flow, k)
    n = np.arange(size, dtype=np.float32)
    return _top_left(np.float32(k) * flow[:, axis] + (n[None, None, :] if axis == 0 else n[None, :, None]), size)


def warp64(frm, flow, k):
    """warpingUnit(frm, flow, k): B x C x h x w.  Returns (the blend, the same blend of |taps|), both float64."""
    f = np.asarray(frm, np.float64)
    if flow is None:
        return f, np.abs(f)
    check_flow(flow, k)
    B, C, h, w = f.shape
    assert flow.shape == (B, 2, h, w)
    xl, wx = tap_index(flow, k, 0, w)                                                             # positions in float32, as the kernels
    yt, wy = tap_index(flow, k, 1, h)
    xr, yb = np.minimum(xl + 1, w - 1), np.minimum(yt + 1, h - 1)
    wxr = np.where(xl + 1 <= w - 1, 1.0 - wx, 0.0)                                          # a missing neighbour weighs 0
    wyb = np.where(yt + 1 <= h - 1, 1.0 - wy, 0.0)
    out, mag = np.empty_like(f), np.empty_like(f)
    for b in range(B):
        taps = [(wy[b] * wx[b], f[b][:, yt[b], xl[b]]), (wy[b] * wxr[b], f[b][:, yt[b], xr[b]]),
                (wyb[b] * wx[b], f[b][:, yb[b], xl[b]]), (wyb[b] * wxr[b], f[b][:, yb[b], xr[b]])]
        out[b] = sum(wt[None] * t for wt, t in taps)
        mag[b] = sum(wt[None] * np.abs(t) for wt, t in taps)
    return out, mag


def costvol64(ref, frm, win=9, fwd=True, frm_abs=None):
    """CostVolMulti(win, fwd) of {ref, frm} in float64: (value, S), B x win*win x h x w each.  frm_abs: sum_taps w_t |tap_t| of a warped frm
    (warp64's second result); |frm| when frm is a plain map."""
    assert win % 2 == 1
    r, f = np.asarray(ref, np.float64), np.asarray(frm, np.float64)
    fa = np.abs(f) if frm_abs is None else np.asarray(frm_abs, np.float64)
    B, C, h, w = r.shape
    n = (win - 1) // 2
    pad = ((0, 0), (0, 0), (n, n), (n, n))
    fp, fap, ra = np.pad(f, pad), np.pad(fa, pad), np.abs(r)
    val, S = np.empty((B, win * win, h, w)), np.empty((B, win * win, h, w))
    rows = max(1, 65536 // (C * w))                                # strips of rows that stay in cache: the same sums, several times faster
    for b in range(B):
        for y0 in range(0, h, rows):
            y1 = min(y0 + rows, h)
            for qx in range(-n, n + 1):
                for qy in range(-n, n + 1):
                    d = (qx + n) * win + (qy + n)
                    sx, sy = (qx, qy) if fwd else (-qx, -qy)
                    win_y, win_x = slice(n - sy + y0, n - sy + y1), slice(n - sx, n - sx + w)   # frm[y - sy, x - sx], 0 outside the map
                    val[b, d, y0:y1] = np.einsum("chw,chw->hw", r[b, :, y0:y1], fp[b, :, win_y, win_x])
                    S[b, d, y0:y1] = np.einsum("chw,chw->hw", ra[b, :, y0:y1], fap[b, :, win_y, win_x])
    return val / C, S / C


def warp_costvol64(ref, nbr_future, nbr_past, flow, k, win=9):
    """ops.warp_costvol in float64: (value, S), B x 2*win*win x h x w each, {fwd, bwd} joined."""
    w3, a3 = warp64(nbr_future, flow, k)
    w1, a1 = warp64(nbr_past, flow, -k)
    vf, sf = costvol64(ref, w3, win, True, a3)
    vb, sb = costvol64(ref, w1, win, False, a1)
    return np.concatenate([vf, vb], 1), np.concatenate([sf, sb], 1)


def measure(got, val, S):
    """(worst |got - val| / (2^-24 S) over S > 0, worst |got - val|, got == 0 wherever S == 0); a NaN in got gives an infinite ratio"""
    got = np.asarray(got, np.float64)
    assert got.shape == val.shape == S.shape
    err = np.abs(got - val)
    err = np.where(np.isfinite(err), err, np.inf)
    pos = S > 0
    ratio = float((err[pos] / (U * S[pos])).max()) if pos.any() else 0.0
    return ratio, float(err.max()), bool(np.all(got[~pos] == 0))


def check(got, val, S, C, what):
    """asserts the bar; returns (ratio, worst absolute error) and prints them"""
    ratio, worst, zeros = measure(got, val, S)
    print("%-64s err / (2^-24 S) = %6.2f (bound %3d)  max |err| = %.3g" % (what, ratio, C + 16, worst))
    assert ratio <= C + 16, "%s: error %.2f x 2^-24 S exceeds the bound C + 16 = %d" % (what, ratio, C + 16)
    assert zeros, what + ": a non-zero result where every product is zero"
    return ratio, worst


# ---- the flows and shapes of the tests -----------------------------------------------------------------------------------------------

def edge_targets(h, w, k):
    """(y, x, u, v): pixels whose targets lie far off each of the four sides in either direction (+k future, -k past), and exactly on the last
    column / last row (left tap with weight 1 and no right / bottom neighbour) and between the last two (h, w >= 2)"""
    s = 5.0 / k                                                   # k = 5 * 2^-n: a flow of j * s moves 5 j pixels
    assert s in (1.0, 2.0, 4.0, 8.0)
    jx, jy = min((w - 1) // 5, 4), min((h - 1) // 5, 4)
    ya, xa = (h - 1) // 2, (w - 1) // 2
    ya2, xa2 = (ya + 1 if ya + 1 < h else max(ya - 1, 0)), (xa + 1 if xa + 1 < w else max(xa - 1, 0))
    return [(0, 0, -32, -32), (h - 1, w - 1, 32, 32), (0, w - 1, -32, 32), (h - 1, 0, 32, -32),
            (ya, w - 1 - 5 * jx, jx * s, 0.25), (ya2, w - 1 - 5 * jx, -jx * s, 0.25),
            (h - 1 - 5 * jy, xa, 0.25, jy * s), (h - 1 - 5 * jy, xa2, 0.25, -jy * s),
            # k / 8 < 1 pixel towards the border from the last but one column / row: the last one as a right / bottom neighbour
            (ya, w - 2, 0.125, 0.25), (ya2, w - 2, -0.125, 0.25), (h - 2, xa, 0.25, 0.125), (h - 2, xa2, 0.25, -0.125)]


def make_flow(kind, seed, B, h, w, k):
    """'noise': quantised white noise of deviation 0.8; 'translation': 2 .. 6 pixels per image and axis plus noise; 'none': None.
    Both carry edge_targets in every image."""
    if kind == "none":
        return None
    r = np.random.default_rng(seed)
    if kind == "noise":
        f = r.standard_normal((B, 2, h, w)) * 0.8
    else:
        assert kind == "translation"
        t = r.uniform(2.0, 6.0, (B, 2, 1, 1)) * r.choice([-1.0, 1.0], (B, 2, 1, 1))
        f = t / k + 0.15 * r.standard_normal((B, 2, h, w))
    f = quantise(f)
    for (y, x, u, v) in edge_targets(h, w, k):
        f[:, 0, y, x] = u
        f[:, 1, y, x] = v
    check_flow(f, k)
    return f


FLOW_KINDS = ("noise", "translation", "none")


def make_maps(seed, B, C, h, w):
    r = np.random.default_rng(seed)
    return [r.standard_normal((B, C, h, w), dtype=np.float32) for _ in range(3)]      # ref, future, past


def tiles(h, w, th, tw):
    return ((h + th - 1) // th) * ((w + tw - 1) // tw)


def auto_variant(n_cu, B, C, h, w):
    """The automatic rule of choose_corr_variant (csrc/b2f_corr.hip) restated for the test's own shapes: what each was built to reach.
    C: the channel count the launcher sees (padded to a multiple of 8)."""
    g2, grid, round2 = tiles(h, w, 16, 16) * B, tiles(h, w, 8, 16) * B, 15 * n_cu // 4
    unit = C % 16 == 0 and h <= 4096 and w <= 4096
    if (h * w <= 2048 or 2 * g2 < round2) and unit:
        return 7
    return 3 if 2 * g2 >= round2 else 1 if grid <= 2 * n_cu else 0


def shapes(n_cu):
    """(name, C, B, h, w, k, branch): the smallest shapes that reach each thing; branch names the launcher branch a shape was built for
    (None: not a shape of the automatic rule) and is asserted against ops.cv_variant on the GPU."""
    def by_launch(B, h, w):       # where the unit kernels do not serve the map or the channel count
        if 2 * tiles(h, w, 16, 16) * B >= 15 * n_cu // 4:
            return "launch fills the two-pixel kernel's round: 3"
        return "grid <= 2 n_cu: 1" if tiles(h, w, 8, 16) * B <= 2 * n_cu else "grid > 2 n_cu, below the two-pixel threshold: 0"
    out = [("interior-16x16", 32, 2, 50, 70, 5.0, None), ("interior-8x16", 48, 1, 49, 35, 2.5, None),
           ("bits-wide", 16, 1, 3, 4096, 0.625, None), ("bits-tall", 16, 1, 4096, 3, 0.625, None),
           ("wide-4097", 16, 1, 2, 4097, 0.625, "the unit kernels refuse the map, " + by_launch(1, 2, 4097)),
           ("tall-4097", 16, 1, 4097, 2, 0.625, "the unit kernels refuse the map, " + by_launch(1, 4097, 2)),
           ("small-map", 32, 2, 24, 40, 2.5, "h*w <= 2048: 7"), ("small-launch", 64, 1, 48, 64, 1.25, "h*w > 2048, small launch: 7")]
    big_b = -(-(15 * n_cu // 4) // (2 * tiles(256, 240, 16, 16)))                  # 2 * tiles16 * B >= 15 n_cu / 4
    out.append(("full-round", 16, big_b, 256, 240, 0.625, "launch fills the two-pixel kernel's round: 3"))
    out.append(("full-round-c8", 8, big_b, 256, 240, 0.625, "launch fills the two-pixel kernel's round: 3"))
    # 8 x 16 tiles of one row and one column each: grid = 2 (n_cu + 1) > 2 n_cu, 2 * tiles16 = 2 (n_cu + 2) < 15 n_cu / 4
    tall = 8 * n_cu + 1
    for C in (8, 24, 40):
        out.append(("c%d-one-round" % C, C, 2, 20, 35, 2.5, "C not a multiple of 16, grid <= 2 n_cu: 1"))
        out.append(("c%d-mid-launch" % C, C, 1, tall, 17, 1.25, "C not a multiple of 16, grid > 2 n_cu, below the two-pixel threshold: 0"))
    for C, k in ((16, 5.0), (32, 5.0), (64, 2.5), (128, 0.625), (48, 2.5), (96, 1.25), (192, 0.625)):
        out.append(("c%d" % C, C, 2, 17, 33, k, "h*w <= 2048: 7"))
    out.append(("c20-padded", 20, 2, 17, 33, 1.25, "C not a multiple of 16, grid <= 2 n_cu: 1"))
    return out


BRANCH_VARIANT = lambda branch: int(branch.rsplit(": ", 1)[1])
