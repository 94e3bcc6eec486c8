"""Float64 restatements of the small kernels of a forward pass (csrc/b2f_glue.hip, csrc/b2f_seq.hip and the node kernels of the generic
executor, csrc/b2f_graph.hip), the yardsticks and counted bounds they are held to, float32 emulations (same operations, same order), the
mutations that must break the bounds, and the inputs and shapes of tests/test_glue_float64_cpu.py and tests/test_gpu_glue_float64.py.
Helper, no test; numpy / torch on the CPU only.  csrc/ = back2future_amd/csrc/.

Coordinates are part of the specification.  A sampler's position, cell and weights are computed as the kernel computes them, in float32,
one rounding per operation (the library is built with -ffp-contract=off, so numpy float32 reproduces them bit for bit):
  upsampling (b2f_glue.hip:83-90,109-110): r = float(n - 1) / float(2 n - 1), c = r * i2, i1 = (int)c, l1 = c - i1, l0 = 1 - l1, the + 1
  neighbour only where i1 < n - 1;
  warps (b2f_internal.h:252-260, b2f_glue.hip:195-199): c = flow * k + x, clamped to [0, size - 1], floored; w = 1 - (c - floor c) and 1 - w.
What follows the weights -- the products of two weights, the blend, the average, the dot product, the softmax -- is float64 here, so a
cell boundary is never a source of disagreement between the kernel and its reference.

Bound per output: n * 2^-24 * S.  S = the float64 sum of the absolute values of the terms (sum |weight| |tap|, sum |x| / 4,
sum |ref| |frm| / C); n = the float32 roundings on one output's path, counted at the source lines ROUNDINGS names (first order, as
tests/conv_float64.py).  Copies and scale by 2.0 are exact: equality.  The softmax is bounded relatively, see softmax_n."""
import functools
import json
import os

import numpy as np

from tests import conv_float64 as CF

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS_PATH = os.path.join(ROOT, "tests", "golden", "glue_float64_ratios.json")
SEED = 21
MARGIN = 2.0          # kernel figure <= MARGIN x the emulation's: the factor of tests/test_gpu_conv_float64.py, taken over, not measured here

# kernel -> (n, where the roundings are counted)
ROUNDINGS = {
    # o = h0l * (w0l * a + w1l * b) + h1l * (w0l * c + w1l * d): on a's path w0l * a 1, + w1l * b 1, h0l * (.) 1, + h1l * (.) 1
    "upsample": (4, "b2f_glue.hip:96-97"),
    # (a + bb + c + d) / 4.0f: three additions; the division by 4 is exact
    "avgpool": (3, "b2f_glue.hip:496-499"),
    # copies (RGB, five zeros)
    "pack": (0, "b2f_glue.hip:22-28"),
    # ColorNormalize: x + (-mean) 1, the correctly rounded quotient by std 1
    "pack-norm": (2, "b2f_glue.hip:23, b2f_internal.h:187-191"),
    # w00 = wx * wy 1; w00 * tl 1; three additions, left to right 3
    "warp": (5, "b2f_glue.hip:207-210 (warp_image_planar), :458,467 (warp_input_planar), b2f_seq.hip:122,131 (warp_input_seq)"),
    # the same on taps that went through ColorNormalize 2
    "warp-norm": (7, "b2f_glue.hip:463-467, b2f_seq.hip:127-131, b2f_internal.h:187-191"),
    # wx * wy * tl + (1.f - wx) * wy * tr + ...: (wx * wy) 1, * tl 1, three additions 3
    "warp_cp8": (5, "b2f_graph.hip:113"),
    # an fmaf chain over C products, one rounding each (n = C + this row's 1: the division by C)
    "costvol_cp8": (1, "b2f_graph.hip:68,71,77,80; per channel 1"),
    # vf + vb of the rounded halves: asserted on bits
    "costvol_cp8-sum": (1, "b2f_graph.hip:84"),
    "add_flow": (1, "b2f_graph.hip:122"),
    # p * 2.0f is exact
    "scale": (0, "b2f_graph.hip:129"),
    "layout": (0, "b2f_glue.hip:521,542,561"),
    "put_channels": (0, "b2f_graph.hip:38-41"),
    # the first layer's row of tests/conv_float64.py ('F1': 9 per channel + 4): the sequence kernel repeats conv_first_kernel's operations
    "conv_first_seq": (CF.n_roundings("F1", 3), "b2f_seq.hip:63-68,77-92; conv_float64.ROUNDINGS['F1']"),
}
# softmax: z - m is float32 (the operand of expf, like a coordinate); e = expf(z - m) within E ulp each, sum 1, quotient 1: p0 = e0 / (e0 + e1)
# is off by at most (E + (E + 1) + 1) u p0 < (2 E + 3) u p0 (b2f_glue.hip:167-170, b2f_graph.hip:145-150).  E is counted in units of
# 2^-24 |exp| (never less than the error in ulp), measured against float64 exp on the test's own z - m where exp is a normal float32
# number; below 2^-126 float32 has no relative precision (and a flushed subnormal is off by up to 2^-126), which the bound adds.
TINY = 2.0 ** -126


def n_of(kernel, C=0):
    return ROUNDINGS[kernel][0] + (C if kernel == "costvol_cp8" else 0)


def measure(got, val, S):
    """worst |got - val| / (2^-24 S) over S > 0 (a NaN in got: inf); where S == 0 got must be 0 (else inf)"""
    got = np.asarray(got, f64)
    assert got.shape == val.shape == S.shape, (got.shape, val.shape, S.shape)
    r = CF.measure(got, val, S)[0]
    if not np.all(got[S == 0] == 0):
        return float("inf")
    return r


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("gauss", "dc", "ramp", "outlier", "integers")


def field(family, shape, salt=0):
    """A float32 array whose last two axes are a map.  gauss: N(0, 1).  dc: + 10 (weights that do not sum to one show).  ramp: a y + b x + c
    per leading index (bilinear x2 of a ramp is the ramp).  outlier: 1 % of the elements (at least one) x 1e4 (a wrong index shows at
    full size).  integers: -8 .. 8."""
    shape = tuple(int(s) for s in shape)
    r = np.random.default_rng([SEED, FAMILIES.index(family), salt] + list(shape))
    if family == "integers":
        return r.integers(-8, 9, shape).astype(f32)
    if family == "ramp":
        return ramp(shape, salt, np.arange(shape[-2], dtype=f64), np.arange(shape[-1], dtype=f64)).astype(f32)
    x = r.standard_normal(shape, dtype=f32)
    if family == "dc":
        x = (x + f32(10)).astype(f32)
    elif family == "outlier":
        flat = x.reshape(-1)
        idx = r.permutation(flat.size)[:max(1, flat.size // 100)]
        flat[idx] *= f32(1e4)
    return x


def ramp(shape, salt, ys, xs):
    """the linear field of field('ramp', shape, salt), a y + b x + c per leading index, at the positions ys x xs in float64"""
    shape = tuple(int(v) for v in shape)
    r = np.random.default_rng([SEED, FAMILIES.index("ramp"), salt] + list(shape))
    a, b, c = (r.standard_normal(shape[:-2] + (1, 1)) for _ in range(3))
    return a * np.asarray(ys, f64)[:, None] + b * np.asarray(xs, f64)[None, :] + c


def records(planar, ps):
    """B x C x h x w -> B x h x w x ps records, the slots from C on hold NaN: a kernel that reads a slot it does not own turns its output NaN"""
    B, C, h, w = planar.shape
    rec = np.full((B, h, w, ps), np.nan, f32)
    rec[..., :C] = np.moveaxis(planar, 1, 3)
    return rec


def to_cp8(planar, fill=np.nan):
    """B x C x h x w -> chunk-planar B x ceil(C / 8) x h x w x 8, the padding channels hold `fill`"""
    B, C, h, w = planar.shape
    ch = (C + 7) // 8
    out = np.full((B, ch * 8, h, w), fill, f32)
    out[:, :C] = planar
    return np.ascontiguousarray(np.moveaxis(out.reshape(B, ch, 8, h, w), 2, 4))


def from_cp8(cp, C):
    B, ch, h, w, _ = cp.shape
    return np.moveaxis(cp, 4, 2).reshape(B, ch * 8, h, w)[:, :C]


# ---- upsampling (nn.SpatialUpSamplingBilinear(2), pwc.lua:360-381) ---------------------------------------------------------------------

UPSAMPLE_SHAPES = [(1, 1), (1, 2), (2, 1),        # smallest maps
                   (3, 5),                        # scalar stores, a tail group of 2
                   (4, 6),                        # 16-byte stores
                   (5, 7),                        # scalar stores, a tail of 2
                   (2, 514),                      # 257 x-groups: the second block in x
                   (2, 513),                      # the same on the scalar path
                   (32767, 1)]                    # the last legal gridDim.y
UPSAMPLE_REFUSED = (32768, 1)
UPSAMPLE_BATCHES = (1, 3)
# the shapes at which `integers` is exact (the float64 reference is a float32 array and the emulation gives it), derived by
# tests/test_glue_float64_cpu.py from the emulation and held to this constant: (h - 1) / (2 h - 1) is a float32 number for h = 1 only, so
# h = w = 1 qualifies; and (32767, 1), where c = r * i has 15 integer bits, which leaves the weights 9 bits: products with -8 .. 8 are exact
UPSAMPLE_EXACT = [(1, 1), (32767, 1)]


def up_axis(n, mutate=None):
    """(i1, neighbour, l0, l1) of the 2 n outputs along one axis, float32 as b2f_glue.hip:83-90,109-110"""
    N2 = 2 * n
    r = f32(n - 1) / f32(N2 - 1)
    if mutate == "ratio":                       # h / H2 where (h - 1) / (H2 - 1) belongs
        r = f32(n) / f32(N2)
    c = (r * np.arange(N2, dtype=f32)).astype(f32)
    i1 = c.astype(np.int64)
    nb = i1 + 1 if mutate == "noclamp" else i1 + (i1 < n - 1)                  # noclamp: see upsample
    l1 = (c - i1.astype(f32)).astype(f32)
    return i1, nb, (f32(1) - l1).astype(f32), l1


def upsample(x, mode="64", mutate=None):
    """x: B x 2 x h x w float32 -> B x 2 x 2h x 2w.  mode '64': the reference; 'abs': S; '32': the emulation (mutate: 'ratio', 'noclamp' (wraps on in memory),
    'swap-scalar' / 'swap-vector': u and v swapped on the scalar / 16-byte store path, 'tail': the tail group's min(x0 + k, W2 - 1) off by one)"""
    B, two, h, w = x.shape
    assert two == 2
    axis_mut = mutate if mutate in ("ratio", "noclamp") else None
    y0, y1, h0, h1 = up_axis(h, axis_mut)
    x0, x1, w0, w1 = up_axis(w, axis_mut)
    wd = f32 if mode == "32" else f64
    X = x.astype(wd)
    if mode == "abs":
        X = np.abs(X)
    if mutate == "noclamp":
        # the + 1 neighbour of the last row / column without its clamp: what lies behind in memory -- the next row's first pixel, the next
        # image's first row, and behind the last image the NaN the op entries' buffers are guarded with.  Its weight is exactly 0 at every
        # size (c = r * (2 n - 1) never exceeds n - 1 in float32), so only that NaN can show: 0 * NaN
        P = np.concatenate([np.moveaxis(X, 1, 3).reshape(B * h * w, 2), np.full((w + 2, 2), np.nan, wd)])
        base = (np.arange(B)[:, None, None] * h + y0[None, :, None]) * w
        g = lambda yy, xx: np.moveaxis(P[base + (yy - y0)[None, :, None] * w + xx[None, None, :]], 3, 1)
    else:
        g = lambda yy, xx: X[:, :, yy][:, :, :, xx]
    h0, h1, w0, w1 = h0.astype(wd)[:, None], h1.astype(wd)[:, None], w0.astype(wd)[None, :], w1.astype(wd)[None, :]
    top = w0 * g(y0, x0) + w1 * g(y0, x1)
    bot = w0 * g(y1, x0) + w1 * g(y1, x1)
    out = h0 * top + h1 * bot
    assert out.dtype == wd
    scalar = (2 * w) & 3
    if (mutate == "swap-scalar" and scalar) or (mutate == "swap-vector" and not scalar):
        out = out[:, ::-1].copy()
    if mutate == "tail":
        out[..., -1] = out[..., -2]
    return out


@functools.lru_cache(maxsize=None)
def upsample_case(family, B, h, w):
    """(x planar, value, S), computed once and shared (read-only)"""
    x = field(family, (B, 2, h, w))
    out = (x, upsample(x, "64"), upsample(x, "abs"))
    for a in out:
        a.setflags(write=False)
    return out


# ---- softmax + nearest upsampling (pwc.lua:308-321) ------------------------------------------------------------------------------------

SOFTMAX_SHAPES = [(1, 1), (5, 3), (2, 257)]
SOFTMAX_BATCHES = (1, 2)
SOFTMAX_REFUSED = (16384, 1)            # 4 h > 65535


def softmax_logits(B, h, w):
    """B x 2 x h x w: Gaussian x 1 and x 30, pairs 88 and 104 apart (exp(-88) is a subnormal float32, exp(-104) underflows) and at +-88,
    +-104, and equal pairs, mixed by a seeded draw; pixel 0 holds an equal pair"""
    r = np.random.default_rng([SEED, 99, B, h, w])
    z = r.standard_normal((B, 2, h, w)).astype(f32)
    cls = r.integers(0, 8, (B, h, w))
    cls.reshape(-1)[0] = 7
    z = np.where(cls[:, None] == 1, z * f32(30), z)
    z[:, 1] = np.where(cls == 2, z[:, 0] - f32(88), z[:, 1])
    z[:, 0] = np.where(cls == 3, z[:, 1] - f32(104), z[:, 0])
    for k, (a, b) in {4: (88.0, -88.0), 5: (-104.0, 104.0)}.items():
        z[:, 0] = np.where(cls == k, f32(a), z[:, 0])
        z[:, 1] = np.where(cls == k, f32(b), z[:, 1])
    z[:, 1] = np.where(cls >= 6, z[:, 0], z[:, 1])
    return z.astype(f32), cls


def softmax_args(z):
    """z - max(z) per pixel in float32, the operands of expf: B x 2 x h x w"""
    m = np.maximum(z[:, 0], z[:, 1])
    return (z - m[:, None]).astype(f32)


def softmax(z, mode="64", mutate=None):
    """z: B x 2 x h x w float32 logits -> probabilities B x 2 x h x w ('64' reference, '32' emulation with a correctly rounded expf;
    mutate 'planes': the two planes swapped)"""
    d = softmax_args(z)
    if mode == "32":
        e = np.exp(d.astype(f64)).astype(f32)          # a correctly rounded expf: the same bits on every host, which numpy's float32 exp is not
        p = (e / (e[:, 0] + e[:, 1])[:, None]).astype(f32)
    else:
        e = np.exp(d.astype(f64))
        p = e / (e[:, 0] + e[:, 1])[:, None]
    return p[:, ::-1].copy() if mutate == "planes" else p


def nearest(p, f):
    return np.repeat(np.repeat(p, f, 2), f, 3)


def exp_error(args32, got32):
    """E of an expf: the worst |got - exp| / (2^-24 exp) against float64 exp over the arguments whose exp is a normal float32 number"""
    a = np.asarray(args32, f32).astype(f64).reshape(-1)
    want = np.exp(a)
    ok = want >= TINY
    return float((np.abs(np.asarray(got32, f64).reshape(-1)[ok] - want[ok]) / (U * want[ok])).max())


def softmax_ratio(got, p64):
    """worst |got - p| / (2^-24 p + 2^-126): the softmax's figure, to be held against softmax_n(E)"""
    err = np.abs(np.asarray(got, f64) - p64)
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / (U * p64 + TINY)).max())


def softmax_n(E_measured):
    """(2 E + 3) with E = twice the measured figure of the expf that ran"""
    return 2.0 * (2.0 * E_measured) + 3.0


# ---- average pooling, packing -----------------------------------------------------------------------------------------------------------

AVGPOOL_SHAPES = [(2, 2), (6, 10), (7, 9)]          # (7, 9): odd, the last row and column are ignored
AVGPOOL_NIMG = (1, 6)


def avgpool(x, mode="64", mutate=None):
    """x: n x H x W x C -> n x H/2 x W/2 x C; mutate 'tap': the fourth tap dropped"""
    n, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    wd = f32 if mode == "32" else f64
    X = np.abs(x.astype(wd)) if mode == "abs" else x.astype(wd)
    a, b = X[:, 0:2 * Ho:2, 0:2 * Wo:2], X[:, 0:2 * Ho:2, 1:2 * Wo:2]
    c, d = X[:, 1:2 * Ho:2, 0:2 * Wo:2], X[:, 1:2 * Ho:2, 1:2 * Wo:2]
    s = a + b + c if mutate == "tap" else a + b + c + d
    return s / wd(4)


def avgpool_input(family, nimg, H, W):
    return np.ascontiguousarray(np.moveaxis(field(family, (nimg, 8, H, W)), 1, 3))


PACK_SHAPES = [(1, 1), (5, 7)]
CN_MEAN, CN_STD = CF.CN_MEAN, CF.CN_STD


def normalize(x, mode="64", axis=1):
    """ColorNormalize of planes c = index % 3 along `axis`: '64' with the kernel's float32 constants in float64; '32': x + (-mean) and the
    correctly rounded quotient, one rounding each (b2f_internal.h:187-191)"""
    sh = [1] * x.ndim
    sh[axis] = x.shape[axis]
    c = np.arange(x.shape[axis]) % 3
    if mode == "32":
        return ((x.astype(f32) + (-CN_MEAN[c]).reshape(sh)).astype(f32) / CN_STD[c].reshape(sh)).astype(f32)
    return (x.astype(f64) - CN_MEAN[c].astype(f64).reshape(sh)) / CN_STD[c].astype(f64).reshape(sh)


def pack(x9, norm, mode="64"):
    """x9: B x 9 x H x W -> 3 x B x H x W x 8 (frame-major; RGB, then five zeros)"""
    B, nine, H, W = x9.shape
    v = normalize(x9, mode) if norm else x9.astype(f32 if mode == "32" else f64)
    out = np.zeros((3, B, H, W, 8), v.dtype)
    for f in range(3):
        out[f, ..., :3] = np.moveaxis(v[:, 3 * f:3 * f + 3], 1, 3)
    return out


# ---- the bilinear sampler (nn.BilinearSamplerBHWD, CUDA semantics) ---------------------------------------------------------------------------

WARP_SHAPES = [(1, 1), (1, 9), (9, 1), (6, 10), (17, 33)]
WARP_BATCHES = (1, 3)
WARP_K = (-20.0, 20.0, 2.5)


def warp_flow(family, B, H, W, k):
    """B x 2 x H x W float32, finite.  integers: multiples of 1.25 / |k| (0.0625 or 0.5: exact), so that every coordinate is a multiple of 1/4,
    every weight one of 1/4 .. 1 and every product exact.  Otherwise one field mixing, by a seeded draw per pixel and component: zero (the
    output is the input), shifts by multiples of 5 pixels (5 / k is exact: a clamped copy), half-pixel targets (+-2.5 pixels), literal
    +-0.5, targets exactly on the last column / row (where the distance is a multiple of 5 pixels), -1e-8 (clamps to 0 in column / row 0),
    +-1e6 (both clamps), and a Gaussian of 3 pixels.  (cls: the draw, B x 2 x H x W.)"""
    r = np.random.default_rng([SEED, 7, FAMILIES.index(family), B, H, W, int(abs(k) * 10), int(k < 0)])
    if family == "integers":
        return (r.integers(-16, 17, (B, 2, H, W)) * (1.25 / abs(k))).astype(f32), None
    fl = (r.standard_normal((B, 2, H, W)) * 3.0 / abs(k)).astype(f32)
    cls = r.integers(0, 9, (B, 2, H, W))
    cls[:, :, 0, 0] = 5
    cls[:, :, H - 1, W - 1] = 4
    sgn = r.choice([-1.0, 1.0], (B, 2, H, W))
    fl[cls == 0] = 0
    fl = np.where(cls == 1, r.integers(-2, 3, fl.shape) * (5.0 / k), fl)
    fl = np.where(cls == 2, sgn * (2.5 / k), fl)
    fl = np.where(cls == 3, sgn * 0.5, fl)
    pos = np.stack(np.broadcast_arrays(np.arange(W)[None, :], np.arange(H)[:, None]), 0)[None]          # 1 x 2 x H x W: x, y
    dist = np.array([W - 1, H - 1]).reshape(1, 2, 1, 1) - pos
    edge = (cls == 4) & (dist % 5 == 0)
    fl = np.where(edge, (dist // 5) * (5.0 / k), fl)
    cls = np.where((cls == 4) & ~edge, 8, cls)
    fl = np.where(cls == 5, -1e-8, fl)
    fl = np.where(cls == 6, sgn * 1e6, fl)
    fl = fl.astype(f32)
    assert np.isfinite(fl).all()
    return fl, cls


def top_left(c, size, mutate=None):
    """bhwd_top_left (b2f_internal.h:252-260) in float32: (index, weight of the top / left tap); mutate 'frac': frac where 1 - frac belongs"""
    assert c.dtype == f32
    c = np.minimum(np.maximum(c, f32(0)), f32(size - 1))
    fl = np.floor(c)
    frac = (c - fl).astype(f32)
    return fl.astype(np.int64), (frac if mutate == "frac" else (f32(1) - frac).astype(f32))


def warp(img, flow, k, mode="64", mutate=None):
    """warpingUnit(img, k * flow): img B x C x H x W (the sample VALUES: float32 for '32', any for '64' / 'abs'), flow B x 2 x H x W planar
    float32.  The coordinates and the four weights wx, wy, 1 - wx, 1 - wy are float32; products of weights, taps and sums are float64 ('64',
    'abs') or float32 in the kernels' order ('32').  A missing right / bottom neighbour has weight exactly 0 (index W - 1 is reached only
    through the clamp, with weight 1), so it is read from the pixel itself.  mutate: 'sign' (k negated), 'frac'."""
    B, C, H, W = img.shape
    kk = f32(-k if mutate == "sign" else k)
    cx = ((flow[:, 0] * kk).astype(f32) + np.arange(W, dtype=f32)[None, None, :]).astype(f32)
    cy = ((flow[:, 1] * kk).astype(f32) + np.arange(H, dtype=f32)[None, :, None]).astype(f32)
    xl, wx = top_left(cx, W, mutate)
    yt, wy = top_left(cy, H, mutate)
    xr, yb = np.minimum(xl + 1, W - 1), np.minimum(yt + 1, H - 1)
    wd = f32 if mode == "32" else f64
    ux, uy = (f32(1) - wx).astype(f32).astype(wd), (f32(1) - wy).astype(f32).astype(wd)
    wx, wy = wx.astype(wd), wy.astype(wd)
    X = np.abs(img.astype(wd)) if mode == "abs" else img.astype(wd)
    out = np.empty((B, C, H, W), wd)
    for b in range(B):
        tl, tr, bl, br = X[b][:, yt[b], xl[b]], X[b][:, yt[b], xr[b]], X[b][:, yb[b], xl[b]], X[b][:, yb[b], xr[b]]
        out[b] = (wx[b] * wy[b])[None] * tl + (ux[b] * wy[b])[None] * tr + (wx[b] * uy[b])[None] * bl + (ux[b] * uy[b])[None] * br
    assert out.dtype == wd
    return out


def unit_of_u8(k8):
    """the float32 value of a byte sample: the correctly rounded k / 255 (b2f_seq.hip:16)"""
    return (k8.astype(f32) / f32(255)).astype(f32)


def image_frames(family, B, H, W):
    """x9: B x 9 x H x W float32 of the family (frame f in planes 3 f .. 3 f + 2)"""
    return field(family, (B, 9, H, W), salt=3)


def byte_frames(n, H, W, salt=0):
    return np.random.default_rng([SEED, 255, salt, n, H, W]).integers(0, 256, (n, 3, H, W)).astype(np.uint8)


# ---- the first layer on a sequence -------------------------------------------------------------------------------------------------------

FIRST_SEQ_T = 4
# one output column, a ragged tile, exactly one tile, one past it, the column-64 staging (ok64) with a second tile
FIRST_SEQ_SHAPES = [(H, W) for H in (2, 14, 16, 18) for W in (2, 62, 64, 66, 130)]


def first_seq_weights():
    _, w, b = CF.make_case("gauss", SEED, 1, 3, 16, 2, 2)
    return w, b


def first32(xn, w, b, mutate=None, raw_pad=None):
    """conv(3, 16, s2) + LeakyReLU in float32 from the bias, taps in (c, ky, kx) order, product and sum rounded (conv_float64.direct32's
    bias-first chain).  xn: T x 3 x H x W normalised samples; the padding is zero -- mutate 'pad': the value raw_pad[c] (ColorNormalize
    applied after the zero padding instead of before it)."""
    T, _, H, W = xn.shape
    Ho, Wo = H // 2, W // 2
    xp = np.zeros((T, 3, H + 2, W + 2), f32)
    if mutate == "pad":
        xp += raw_pad.reshape(1, 3, 1, 1)
    xp[:, :, 1:-1, 1:-1] = xn
    acc = np.zeros((T, 16, Ho, Wo), f32) + b.astype(f32)[None, :, None, None]
    for c in range(3):
        for ky in range(3):
            for kx in range(3):
                win = xp[:, c, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
                acc = (acc + (w[None, :, c, ky, kx, None, None] * win[:, None]).astype(f32)).astype(f32)
    return np.maximum(acc, (f32(0.2) * acc).astype(f32))


# ---- layout, put_channels ------------------------------------------------------------------------------------------------------------------

LAYOUT_C = (2, 3, 81, 162)
LAYOUT_HW = [(1, 1), (5, 7)]
PUT_C_OFF = (0, 2, 81, 13)
PUT_C = (2, 25, 81)


def put_channels(src_planar, dst_cp8, c_off, mutate=None):
    """C channels of src (B x C x hw-map planar) into channels c_off .. of a copy of the chunk-planar dst; mutate 'c_off8': c_off rounded down to 8"""
    out = dst_cp8.copy()
    B, ch, h, w, _ = out.shape
    v = np.moveaxis(out, 4, 2).reshape(B, ch * 8, h, w).copy()
    o = (c_off // 8) * 8 if mutate == "c_off8" else c_off
    v[:, o:o + src_planar.shape[1]] = src_planar
    return np.ascontiguousarray(np.moveaxis(v.reshape(B, ch, 8, h, w), 2, 4))


# ---- the executor's cost volume ------------------------------------------------------------------------------------------------------------

COSTVOL_WIN = (1, 3, 5, 9, 15)
COSTVOL_C = (3, 16, 20)
COSTVOL_HW = [(1, 1), (3, 4), (9, 7)]          # maps smaller than the window


def costvol(ref, frm, win, fwd, mode="64", mutate=None):
    """CostVolMulti(win, fwd){ref, frm} (CostVolMulti.lua:49-109, costvol_cp8_kernel): channel d = (qx + n) * win + (qy + n); fwd reads
    frm[y - qy, x - qx], bwd frm[y + qy, x + qx]; out of range 0; / C.  '64' / 'abs' float64; '32': an fma chain in channel order (the
    product exact, the sum rounded: in float64, then to float32), then the float32 quotient.  mutate: 'transpose' (qx and qy exchanged),
    'bwd-y' (the backward direction read at y - qy)."""
    B, C, h, w = ref.shape
    n = (win - 1) // 2
    R, Fm = ref.astype(f64), frm.astype(f64)
    if mode == "abs":
        R, Fm = np.abs(R), np.abs(Fm)
    Fp = np.pad(Fm, ((0, 0), (0, 0), (n, n), (n, n)))
    out = np.empty((B, win * win, h, w), f32 if mode == "32" else f64)
    for d in range(win * win):
        qx, qy = d // win - n, d % win - n
        if mutate == "transpose":
            qx, qy = qy, qx
        sx, sy = (-qx, -qy) if fwd else (qx, qy)
        if mutate == "bwd-y" and not fwd:
            sy = -qy
        nb = Fp[:, :, n + sy:n + sy + h, n + sx:n + sx + w]
        if mode == "32":
            a = np.zeros((B, h, w), f32)
            for c in range(C):
                a = (a.astype(f64) + R[:, c] * nb[:, c]).astype(f32)
            out[:, d] = (a / f32(C)).astype(f32)
        else:
            out[:, d] = (R * nb).sum(1) / C
    return out


def costvol_maps(family, B, C, h, w):
    """ref, frmF, frmB: B x C x h x w"""
    return [field(family, (B, C, h, w), salt=10 + i) for i in range(3)]


# ---- the emulation's ratios ----------------------------------------------------------------------------------------------------------------

def _worst(rs):
    return float(max(rs)) if rs else 0.0


def _pair(r, n):
    return (r, r / n if n else (0.0 if r == 0 else float("inf")))


def first_seq_case(family, H, W, kind):
    """(x as handed to the entry: float32 or uint8 T x 3 x H x W, the float32 sample values before ColorNormalize, normalize?)"""
    if kind == "u8":
        x = byte_frames(FIRST_SEQ_T, H, W)
        return x, unit_of_u8(x), True
    x = field(family, (FIRST_SEQ_T, 3, H, W), salt=5)
    return x, x, kind == "unit"


def first_seq_reference(vals, norm, w, b):
    x64 = normalize(vals, "64") if norm else vals.astype(f64)
    return CF.conv64(x64, w, b, 2, True), CF.S_direct(x64, w, b, 2)


def first_seq_emulation(vals, norm, w, b, mutate=None):
    xn = normalize(vals, "32") if norm else vals
    return first32(xn, w, b, mutate, normalize(np.zeros((1, 3, 1, 1), f32), "32").reshape(3) if mutate == "pad" else None)


def emulation_ratios(kernel, family, mutate=None):
    """(worst err / (2^-24 S), worst err / bound) of the float32 emulation of `kernel` over the shapes of the GPU file on one family (softmax:
    err / (2^-24 p + 2^-126) and that over softmax_n of the emulation's correctly rounded expf, family 'logits'); mutate: the emulation's mutation"""
    rs = []
    n_fixed = n_of(BOUND_OF.get(kernel, kernel)) if kernel != "softmax" else 1
    if kernel == "upsample":
        for (h, w) in UPSAMPLE_SHAPES:
            for B in UPSAMPLE_BATCHES:
                x, val, S = upsample_case(family, B, h, w)
                rs.append(_pair(measure(upsample(x, "32", mutate), val, S), n_fixed))
    elif kernel == "softmax":
        for (h, w) in SOFTMAX_SHAPES:
            for B in SOFTMAX_BATCHES:
                z, _ = softmax_logits(B, h, w)
                d = softmax_args(z)
                rs.append(_pair(softmax_ratio(softmax(z, "32", mutate), softmax(z, "64")), softmax_n(exp_error(d, np.exp(d.astype(f64)).astype(f32)))))
    elif kernel == "avgpool":
        for (H, W) in AVGPOOL_SHAPES:
            for n in AVGPOOL_NIMG:
                x = avgpool_input(family, n, H, W)
                rs.append(_pair(measure(avgpool(x, "32", mutate), avgpool(x, "64"), avgpool(x, "abs")), n_fixed))
    elif kernel == "pack-norm":
        for (H, W) in PACK_SHAPES:
            x9 = image_frames(family, 2, H, W)
            val = pack(x9, True, "64")
            rs.append(_pair(measure(pack(x9, True, "32"), val, np.abs(val)), n_fixed))
    elif kernel in ("warp", "warp-norm", "warp-u8", "warp_cp8"):
        for (H, W) in WARP_SHAPES:
            for B in WARP_BATCHES:
                for k in WARP_K:
                    flow, _ = warp_flow(family, B, H, W, k)
                    if kernel == "warp_cp8":
                        img = field(family, (B, 24, H, W), salt=4)
                    elif kernel == "warp-u8":
                        img = unit_of_u8(byte_frames(B, H, W, 1))
                    else:
                        img = image_frames(family, B, H, W)[:, :3]
                    norm = kernel in ("warp-norm", "warp-u8")
                    v64 = normalize(img, "64") if norm else img
                    v32 = normalize(img, "32") if norm else img
                    rs.append(_pair(measure(warp(v32, flow, k, "32", mutate), warp(v64, flow, k, "64"), warp(v64, flow, k, "abs")), n_fixed))
    elif kernel == "costvol_cp8":
        for win in COSTVOL_WIN:
            for C in COSTVOL_C:
                for (h, w) in COSTVOL_HW:
                    ref, fF, fB = costvol_maps(family, 2, C, h, w)
                    for fwd, frm in ((True, fF), (False, fB)):
                        r = measure(costvol(ref, frm, win, fwd, "32", mutate), costvol(ref, frm, win, fwd, "64"), costvol(ref, frm, win, fwd, "abs"))
                        rs.append((r, r / n_of("costvol_cp8", C)))
    elif kernel == "add_flow":
        a, b = field(family, (1, 2, 9, 7), salt=20), field(family, (1, 2, 9, 7), salt=21)
        rs.append(_pair(measure((a + b).astype(f32), a.astype(f64) + b.astype(f64), np.abs(a.astype(f64)) + np.abs(b.astype(f64))), n_fixed))
    elif kernel.startswith("first_seq"):
        kind = kernel.split("-")[1]
        w, b = first_seq_weights()
        for (H, W) in FIRST_SEQ_SHAPES:
            _, vals, norm = first_seq_case(family, H, W, kind)
            val, S = first_seq_reference(vals, norm, w, b)
            rs.append(_pair(measure(first_seq_emulation(vals, norm, w, b, mutate), val, S), n_fixed))
    else:
        raise KeyError(kernel)
    return _worst([r[0] for r in rs]), _worst([r[1] for r in rs])


EMULATED = ("upsample", "avgpool", "pack-norm", "warp", "warp-norm", "warp-u8", "warp_cp8", "costvol_cp8", "add_flow", "first_seq-float", "first_seq-unit",
            "first_seq-u8")
# the kernel whose ROUNDINGS row bounds an emulated row
BOUND_OF = {"warp-u8": "warp-norm", "first_seq-float": "conv_first_seq", "first_seq-unit": "conv_first_seq", "first_seq-u8": "conv_first_seq"}


def families_of(kernel):
    return ("bytes",) if kernel.endswith("-u8") else FAMILIES


def compute_ratios():
    out = {k: {fam: emulation_ratios(k, fam if fam != "bytes" else "gauss")[0] for fam in families_of(k)} for k in EMULATED}
    out["softmax"] = {"logits": emulation_ratios("softmax", "logits")[0]}
    return out


@functools.lru_cache(maxsize=None)
def recorded_ratios():
    """tests/golden/glue_float64_ratios.json: compute_ratios() as recorded by `python -m tests.glue_float64`; tests/test_glue_float64_cpu.py
    holds the file to a fresh computation, the GPU file reads it"""
    with open(RATIOS_PATH) as f:
        return json.load(f)


def recorded(kernel, family):
    return recorded_ratios()[kernel][family]


if __name__ == "__main__":
    with open(RATIOS_PATH, "w") as f:
        json.dump(compute_ratios(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(RATIOS_PATH).read())
