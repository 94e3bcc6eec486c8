"""A float64 restatement of the 3x3 convolutions (nn.SpatialConvolution(Ci, Co, 3, 3, s, s, 1, 1) + LeakyReLU(0.2), pwc.lua:58-65,76-85), the
yardsticks their kernels are held to against it on ANY input, float32 emulations of the algorithms, and the inputs and shapes of the tests
that use them (tests/test_conv_float64_cpu.py, tests/test_gpu_conv_float64.py, and the tile-geometry sweep of tests/test_gpu_conv_edges.py:
GEOMETRY, edge_shapes below).  Helper, no test; numpy / torch on the CPU only.

Yardsticks.  u = 2^-24.  S_direct = conv64(|x|, |w|, |b|): the sum of the absolute products of one output.  S_wino(alg) = the same Winograd
algorithm evaluated in float64 on absolute values, |A^T| [sum_ci (|G| |g| |G^T|) .* (|B^T| |d| |B|)] |A| + |b| per output tile (zero padding,
tiles from the map's origin, the ragged last tiles cut): every intermediate of the kernel is bounded by the matching intermediate of that
evaluation, so one rounding anywhere on an output's path moves the output by at most u S_wino.  The error of a Winograd kernel scales
with S_wino, not with S_direct (F(4x4): S_wino / S_direct ~ 60, F(6x6): ~ 225), and on inputs with a DC offset, one-sided activations or a
few large channels the two are no longer proportional to the output.

bound(tag, Ci_padded, S) = n(tag) * u * S, first order, n = the number of float32 roundings on one output's path, counted at the source
lines named in ROUNDINGS below (csrc/ = back2future_amd/csrc/).  Ci_padded: the channels the kernel multiplies (chunks of 8).
The split-operand bf16 kernels (E1, E2, L2, V1, the head) write x = h + m + l and w = h + m + l exactly (three bf16 terms: split() of
b2f_w1b.hip:80-90; l fits because |m| <= 2^-8 |v| and |l| <= 2^-16 |v| leave 8 bits) and keep six of the nine term products (Wa Xa + Wb Xa +
Wa Xb = hh + mm + hm + mh + lh + hl, b2f_w1b.hip:21-23).  The products are exact in the MFMA (8 x 8 bits); each of the six is one more
float32 addition into the accumulator, counted as a rounding each whatever order the MFMA adds them in: 6 per product where the fp32
kernel has 1.  The dropped ml + lm + ll is at most (2 * 2^-24 + 2^-32) |x| |w| per product: 3 u S in all, the SPLIT_DROPPED term.

Exactness.  LeakyReLU in every kernel is max(v, 0.2f * v) in float32: where the float64 value v is itself a float32 number (the `integers`
family, an all-zero image) the kernel's result is round32(float64(float32(0.2)) * v), one rounding of an exact product; round32_leaky gives
that number.  It differs from round32(0.2 * v) by at most one ulp, far inside every bound."""
import functools
import importlib.util
import json
import os

import numpy as np
import torch

U = 2.0 ** -24
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS_PATH = os.path.join(ROOT, "tests", "golden", "conv_float64_ratios.json")


@functools.lru_cache(maxsize=None)
def numerics():
    """tools/wino6_numerics.py: the matrices of F(2x2), F(4x4), F(6x6) as the kernels' headers state them (b2f_wino.hip:656, b2f_wino4.hip:7-9,
    b2f_wino6.hip:6-11, b2f_w1b.hip:213,387,599: the same interpolation points; b2f_wino.hip negates row 2 of B^T and of G, which cancels)"""
    spec = importlib.util.spec_from_file_location("wino6_numerics", os.path.join(ROOT, "tools", "wino6_numerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def matrices(alg):
    """(B^T, G, A^T) of 'F2', 'F4', 'F6'; '1D' (b2f_w1b.hip: F(4,3) along x -- the W axis --, direct along y) uses F4's"""
    N = numerics()
    return {"F2": (N.BT2, N.G2, N.AT2), "F4": (N.BT4, N.G4, N.AT4), "F6": (N.BT6, N.G6, N.AT6), "1D": (N.BT4, N.G4, N.AT4)}[alg]


ALGS = ("direct", "direct-b", "F2", "F4", "F6", "1D")      # direct-b: the accumulator starts at the bias (b2f_conv.hip:162-192)
SLOPE32 = float(f32(0.2))


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------

def conv64(x, w, b, stride=1, leaky=False):
    """3x3 cross-correlation with padding 1 in float64; bias and LeakyReLU(0.2) in float64.  x: B x Ci x H x W, w: Co x Ci x 3 x 3, b: Co."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    y = torch.nn.functional.conv2d(t(x), t(w), t(b), padding=1, stride=stride)
    return (torch.where(y > 0, y, 0.2 * y) if leaky else y).numpy()


def S_direct(x, w, b, stride=1):
    return conv64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64)), stride, False)


def round32_leaky(v64, leaky):
    """float32 of a float64 value that is a float32 number, through the kernels' max(v, 0.2f * v)"""
    v = np.asarray(v64, np.float64)
    return (np.where(v > 0, v, SLOPE32 * v) if leaky else v).astype(f32)


# ---- Winograd in three arithmetics: float64, float64 on absolute values, float32 in the kernels' order ----------------------------------

def _lin(M, x, axis, mode):
    """y = M x along axis.  '64': float64; 'abs': |M| x; '32': float32, one rounding per multiply and per add, terms in index order (zero
    coefficients skipped) -- at least as many roundings as the kernels' fused chains"""
    if mode != "32":
        return np.moveaxis(np.tensordot(np.abs(M) if mode == "abs" else M, np.moveaxis(x, axis, 0), axes=(1, 0)), 0, axis)
    return numerics().lin32(M, x, axis)


def _bf16(a):
    """float32 -> nearest bf16 (ties to even), as float32"""
    i = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    i = ((i + 0x7FFF + ((i >> 16) & 1)) >> 16) << 16
    return i.astype(np.uint32).view(f32)


def _mutate_w(w, mutate):
    if mutate == "tap":                       # one tap of one input channel dropped
        w = w.copy()
        w[:, min(3, w.shape[1] - 1), 2, 1] = 0
    return w


def _mutate_x(x, mutate):
    if mutate == "swap" and x.shape[1] >= 3:  # two input channels of the first chunk swapped
        x = x.copy()
        x[:, [1, 2]] = x[:, [2, 1]]
    return x


EDGE_MUTATIONS = ("edge-leak", "edge-stale")          # wrong only where the map cuts a tile: see _mutate_halo, _mutate_last_column


def ragged(h, w, tile):
    """(rows, columns): does an h x w OUTPUT map cut its last tile of tile = (th, tw) pixels?"""
    return h % tile[0] != 0, w % tile[1] != 0


def _mutate_halo(xp, H, W, cut, mutate):
    """edge-leak on the zero-padded input xp (the H x W map at [1 : H + 1, 1 : W + 1]): where the last tile is cut (cut = ragged(...) of the
    output map), the first out-of-map column / row holds the clamped in-map value -- the last column / row again -- instead of zero, as a
    loader that clamps its address and forgets the mask leaves it.  The corner stays zero."""
    if mutate == "edge-leak":
        if cut[1]:
            xp[:, :, 1:H + 1, W + 1] = xp[:, :, 1:H + 1, W]
        if cut[0]:
            xp[:, :, H + 1, 1:W + 1] = xp[:, :, H, 1:W + 1]


def _mutate_last_column(out, cut, mutate):
    """edge-stale on the output: the last valid column of a cut last tile takes its left neighbour's output (zero in a one-column map), as a
    store loop that stops one column early leaves it"""
    if mutate == "edge-stale" and cut[1]:
        out[..., -1] = out[..., -2] if out.shape[-1] > 1 else 0
    return out


def winograd(x, w, b, alg, mode, leaky=False, mutate=None):
    """The Winograd algorithm alg ('F2', 'F4', 'F6', '1D') at stride 1 on x: B x Ci x H x W.  mode '64': float64 (reproduces conv64);
    'abs': S_wino; '32': the float32 emulation (U = G g G^T in double rounded once, as the packers; transforms rows first; the K sum in
    channel order, product and sum rounded; bias, then max(v, 0.2f v)).  mutate (mode '32' only): 'bf16' U rounded to bf16, 'tap', 'swap',
    and the two of EDGE_MUTATIONS on the algorithm's own tile (m x m; '1D': 1 x 4)."""
    BT, G, AT = matrices(alg)
    m, n = AT.shape
    one_d = alg == "1D"
    x, w, b = np.asarray(x), _mutate_w(np.asarray(w), mutate), np.asarray(b)
    x = _mutate_x(x, mutate)
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    wd = np.float64 if mode != "32" else f32
    xs, ws, bs = ((np.abs(a.astype(np.float64)) if mode == "abs" else a.astype(np.float64)) for a in (x, w, b))
    ty, tx = (H if one_d else -(-H // m)), -(-W // m)
    hp = H + 2 if one_d else ty * m + 2
    xp = np.zeros((B, Ci, hp, tx * m + 2), wd)
    xp[:, :, 1:H + 1, 1:W + 1] = xs
    cut = ragged(H, W, (1 if one_d else m, m))
    if mode == "32":
        _mutate_halo(xp, H, W, cut, mutate)
    Gm = np.abs(G) if mode == "abs" else G
    if one_d:
        # V[b, c, r, t, xi] = sum_j BT[xi, j] xp[b, c, r, 4 t + j];  Uk[o, c, ky, xi] = sum_kx G[xi, kx] w[o, c, ky, kx]
        d = np.stack([xp[:, :, :, j:j + tx * m:m] for j in range(n)], -1)
        V = _lin(BT, d, 4, mode)
        Uk = np.einsum("ak,ocyk->ocya", Gm, ws).astype(wd)
        if mutate == "bf16":
            Uk = _bf16(Uk)
        if mode == "32":
            M = np.zeros((B, Co, H, tx, n), f32)
            for c in range(Ci):
                for ky in range(3):
                    M = (M + (Uk[None, :, c, ky, None, None, :] * V[:, None, c, ky:ky + H]).astype(f32)).astype(f32)
        else:
            M = sum(np.einsum("oca,bcrta->borta", Uk[:, :, ky], V[:, :, ky:ky + H], optimize=True) for ky in range(3))
        Y = _lin(AT, M, 4, mode)                                               # B x Co x H x tx x m
        out = Y.reshape(B, Co, H, tx * m)[:, :, :, :W]
    else:
        d = np.empty((B, Ci, ty, tx, n, n), wd)
        for i in range(n):
            for j in range(n):
                d[..., i, j] = xp[:, :, i:i + ty * m:m, j:j + tx * m:m]
        V = _lin(BT, _lin(BT, d, 4, mode), 5, mode)
        Uw = np.einsum("ai,ocij,bj->ocab", Gm, ws, Gm).astype(wd)
        if mutate == "bf16":
            Uw = _bf16(Uw)
        if mode == "32":
            M = np.zeros((B, Co, ty, tx, n, n), f32)
            for c in range(Ci):
                M = (M + (Uw[None, :, c, None, None] * V[:, None, c]).astype(f32)).astype(f32)
        else:
            Um = np.moveaxis(Uw, (2, 3), (0, 1))                               # n x n x Co x Ci
            Vm = np.moveaxis(V, (4, 5, 1), (0, 1, 2)).reshape(n, n, Ci, B * ty * tx)
            M = np.moveaxis(np.matmul(Um, Vm).reshape(n, n, Co, B, ty, tx), (0, 1, 2, 3), (4, 5, 1, 0))
        Y = _lin(AT, _lin(AT, M, 5, mode), 4, mode)                            # columns (in registers) first, then rows
        out = np.moveaxis(Y, 4, 3).reshape(B, Co, ty * m, tx * m)[:, :, :H, :W]
    if mode == "32":
        v = _mutate_last_column((out + bs.astype(f32)[None, :, None, None]).astype(f32), cut, mutate)
        return np.maximum(v, (f32(0.2) * v).astype(f32)) if leaky else v
    v = out + bs[None, :, None, None]
    return np.where(v > 0, v, 0.2 * v) if (leaky and mode == "64") else v


def S_wino(x, w, b, alg):
    return winograd(x, w, b, alg, "abs")


def direct32(x, w, b, stride=1, leaky=False, mutate=None, bias_first=False, tile=None):
    """float32 accumulation in channel order (then taps), product and sum rounded: the emulation of the direct kernels.  bias_first: the
    chain starts at the bias instead of ending with it, as conv3x3_mfma's accumulators do (b2f_conv.hip:162-192, "same order as y = b + sum
    in nn"): every partial sum then carries the bias, and with |b| ~ the output's deviation the rounding of the chain about doubles.
    tile = (th, tw) of output pixels: what EDGE_MUTATIONS call a tile here (a direct kernel has none of its own; without it they do nothing)."""
    x, w, b = _mutate_x(np.asarray(x, f32), mutate), _mutate_w(np.asarray(w, f32), mutate), np.asarray(b, f32)
    if mutate == "bf16":
        w = _bf16(w)
    B, Ci, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    cut = ragged(Ho, Wo, tile) if tile else (False, False)
    xp = np.zeros((B, Ci, H + 2, W + 2), f32)
    xp[:, :, 1:-1, 1:-1] = x
    _mutate_halo(xp, H, W, cut, mutate)
    acc = np.zeros((B, w.shape[0], Ho, Wo), f32)
    if bias_first:
        acc += b[None, :, None, None]
        b = np.zeros_like(b)
    for c in range(Ci):
        for ky in range(3):
            for kx in range(3):
                win = xp[:, c, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
                acc = (acc + (w[None, :, c, ky, kx, None, None] * win[:, None]).astype(f32)).astype(f32)
    v = _mutate_last_column((acc + b[None, :, None, None]).astype(f32), cut, mutate)
    return np.maximum(v, (f32(0.2) * v).astype(f32)) if leaky else v


def emulate(alg, x, w, b, stride=1, leaky=False, mutate=None, tile=None):
    if alg in ("direct", "direct-b"):
        return direct32(x, w, b, stride, leaky, mutate, alg == "direct-b", tile)
    return winograd(x, w, b, alg, "32", leaky, mutate)


def yardstick(alg, x, w, b, stride=1):
    return S_direct(x, w, b, stride) if alg in ("direct", "direct-b") else S_wino(x, w, b, alg)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------

SPLIT_DROPPED = 3          # ceil(2 + 2^-8): the three dropped term products, in units of u |x| |w|
# tag -> (algorithm of the yardstick, roundings per multiplied channel, roundings outside the K sum, where they are counted)
ROUNDINGS = {
    # direct fp32 MFMA: an fmaf chain over 9 Ci products, + bias, + 0.2f * v
    "D1": ("direct", 9, 2, "b2f_conv.hip: fp32 MFMA chain, bias, LeakyReLU"), "D2": ("direct", 9, 2, "b2f_conv.hip"),
    "N2": ("direct", 9, 2, "b2f_glue.hip conv_narrow2"), "C16": ("direct", 9, 2, "b2f_conv16.hip"), "S16": ("direct", 9, 2, "b2f_conv16.hip"),
    # F(2x2): U rounded once (b2f_wino.hip:656) 1; B^T d: one fma (:202), (.) B: one add (:203) 2; A^T M A: t0 = a + b + c (:308) 2,
    # mm0 + mm1 + mm2 (:337) 2; + bias (:337) 1; 0.2f * v (:338) 1
    "W2": ("F2", 1, 9, "b2f_wino.hip:202,203,308,337,338,656"), "W2+": ("F2", 1, 9, "b2f_wino.hip (conv3x3_wino8: the same operations)"),
    # F(4x4): U 1 (b2f_wino4.hip:1629); rows P / Q then r = fma(cs, Q, P) (:367-370) 2; columns fma, fma or fma, add (:389-400) 2;
    # A^T M A: s, M0 + s1, + s2 | d2, fma, + M5 (:152-156) 3 and again (:164-169) 3 (wino4_output_half :212-213: fma, fma, fma 3);
    # + bias (:173) 1; 0.2f * v (:174) 1
    "W4": ("F4", 1, 13, "b2f_wino4.hip:152-156,164-174,367-370,389-400,1629"),
    # F(6x6): U 1 (b2f_wino6.hip:815); rows: a 5-fma chain (:471-475) 5; columns: mul, fma, fma, add (:505-511) 4; A^T M A: s, + M0, + s2,
    # + s3 | d, fma, fma, + M7 (:192-211) 4 and fma x 4 (:256-266) 4; slope * v (:280) 1; the bias starts the accumulator of xi = (1, 1)
    # (:171): its addition is the K chain's first, counted 1
    "W6": ("F6", 1, 20, "b2f_wino6.hip:171,192-211,256-266,280,471-475,505-524,815"),
    # 1-D F(4,3) on the bf16 pipe: 3 Ci products of six kept terms each 18; U 1 (b2f_w1b.hip:620); B^T d: fma, fma or fma, add (:224-231) 2;
    # A^T m: s, + m0, + s34, + bias | d, fma, + m5, + bias (:432-436) 4; slope * v (:437) 1; dropped terms 3
    "V1": ("1D", 18, 8 + SPLIT_DROPPED, "b2f_w1b.hip:224-231,432-440,620; split :80-90"),
    # direct on the bf16 pipe: 9 Ci products of six kept terms each 54; bias 1, LeakyReLU 1, dropped terms 3
    "E1": ("direct", 54, 2 + SPLIT_DROPPED, "b2f_convb.hip:6,319"), "E2": ("direct", 54, 2 + SPLIT_DROPPED, "b2f_convb.hip:6,319"),
    "L2": ("direct", 54, 2 + SPLIT_DROPPED, "b2f_s2b.hip:2-3,403"), "HEAD": ("direct", 54, 2 + SPLIT_DROPPED, "b2f_head.hip:19,50 (per layer)"),
    # the first layer: an fmaf chain over 27 products from the bias (b2f_glue.hip:290-300), 0.2f * v (:305) 1, and with ColorNormalize two
    # roundings on every input, x + (-mean) and the IEEE quotient by std (b2f_internal.h:187-191: the correction step makes it the correctly
    # rounded quotient), which multiply every product: 2; without it the count is 2 too many.  Ci_padded = 3: no channel padding.
    "F1": ("direct", 9, 1 + 1 + 2, "b2f_glue.hip:290-305, b2f_internal.h:187-191"),
    # experiments build.  B16: the 16 -> 16 layer on the bf16 pipe (b2f_conv16b.hip), as E1.  W4S / W4H: the 64-output n-blocks of an F(4x4)
    # launch with split operands (wino4_split, b2f_wino4s.hip; wino4_hybrid: some xi steps only -- bounded as if all were): W4's count with
    # six term products per channel, and the dropped terms.  W2S: the same blocks as F(2x2) on the bf16 pipe (wino2_split, b2f_wino2s.hip):
    # W2's count, six per channel, dropped terms.  The last n-block of <= 32 outputs stays on the fp32 F(4x4) kernel (b2f_wino4.hip:1604-1609).
    "B16": ("direct", 54, 2 + SPLIT_DROPPED, "b2f_conv16b.hip"),
    "W4S": ("F4", 6, 13 + SPLIT_DROPPED, "b2f_wino4s.hip, b2f_wino4.hip:1605"), "W4H": ("F4", 6, 13 + SPLIT_DROPPED, "b2f_wino4.hip (HYB)"),
    "W2S": ("F2", 6, 9 + SPLIT_DROPPED, "b2f_wino2s.hip, b2f_wino4.hip:1604"),
}


EMULATION = {"D1": "direct-b", "D2": "direct-b", "F1": "direct-b"}          # the emulation a tag's tight bar reads; every other tag: its yardstick's algorithm


def emulation_of(tag):
    return EMULATION.get(tag, ROUNDINGS[tag][0])


def padded(ci):
    return (ci + 7) // 8 * 8


def n_roundings(tag, ci_padded):
    alg, per_channel, fixed, _ = ROUNDINGS[tag]
    return per_channel * ci_padded + fixed


def bound(tag, ci_padded, S):
    """n * 2^-24 * S: S is the yardstick of ROUNDINGS[tag][0] (S_direct, or S_wino of the algorithm that ran)"""
    return n_roundings(tag, ci_padded) * U * S


def head64(x, w1, b1, w2, b2):
    """conv(16, 16, s1) + LeakyReLU + conv(16, 32, s2) + LeakyReLU in float64: (value, bound).  The first layer's bound E1 passes through the
    LeakyReLU (1-Lipschitz) and the second layer's |w|: bound = n u S2 + conv(E1, |w2|), S2 on the float64 map."""
    t = conv64(x, w1, b1, 1, True)
    e1 = bound("HEAD", 16, S_direct(x, w1, b1, 1))
    y = conv64(t, w2, b2, 2, True)
    return y, bound("HEAD", 16, S_direct(t, w2, b2, 2)) + S_direct(e1, w2, np.zeros_like(b2), 2)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("gauss", "dc", "leaky", "outlier", "decades", "sparse", "integers")


def make_case(family, seed, B, Ci, Co, H, W):
    """(x, w, b) float32 of a seeded generator.  gauss: x ~ N(0, 1), w ~ N(0, 1 / (9 Ci)), b ~ N(0, 1), what every other conv test draws.
    dc: x + 10.  leaky: LeakyReLU(0.2) of x.  outlier: 5 % of the input channels (at least one) and 3 % of the filters (at least one) x 100.
    decades: channel c scaled by 10^U(-3, 3).  sparse: 95 % of x exactly zero, every fourth channel all zero next to a channel x 100, the
    last image all zero, every other bias zero (so that S = 0 occurs).  integers: x in {-8 .. 8}, w in {-4 .. 4} * 2^-3, b in {-8 .. 8}:
    every product is a multiple of 2^-3 below 2^5 and every partial sum of the direct, F(2x2) (U = G g G^T in multiples of 2^-5, V sums
    of four inputs) and split-bf16 (4-bit operands: h alone) paths stays below 2^24 * 2^-5: all exact in float32."""
    r = np.random.default_rng([seed, FAMILIES.index(family), B, Ci, Co, H, W])
    if family == "integers":
        x = r.integers(-8, 9, (B, Ci, H, W)).astype(f32)
        w = (r.integers(-4, 5, (Co, Ci, 3, 3)) / 8.0).astype(f32)
        return x, w, r.integers(-8, 9, Co).astype(f32)
    x = r.standard_normal((B, Ci, H, W), dtype=f32)
    w = (r.standard_normal((Co, Ci, 3, 3), dtype=f32) / np.sqrt(9 * Ci)).astype(f32)
    b = r.standard_normal(Co, dtype=f32)
    if family == "dc":
        x = (x + f32(10)).astype(f32)
    elif family == "leaky":
        x = np.where(x > 0, x, f32(0.2) * x).astype(f32)
    elif family == "outlier":
        x[:, r.permutation(Ci)[:max(1, Ci // 20)]] *= f32(100)
        w[r.permutation(Co)[:max(1, (3 * Co) // 100)]] *= f32(100)
    elif family == "decades":
        x *= (10.0 ** r.uniform(-3, 3, (1, Ci, 1, 1))).astype(f32)
    elif family == "sparse":
        x *= (r.random(x.shape) < 0.05)
        x[:, 1::4] *= f32(100)
        x[:, 0::4] = 0
        x[B - 1] = 0
        b[0::2] = 0
    return x, w, b


# ---- shapes (Ci, Co, H, W of the INPUT), batch 2 ------------------------------------------------------------------------------------------
# outputs 1 x 1; 8 x 16 (one F(2x2) block); 17 x 33 (one past an F(4x4) block both ways); 13 x 49 (one past an F(6x6) 12 x 48 item both ways)
# Ci 32 (even chunk count, wino6's four-chunk minimum), 40 (5 chunks), 72 (odd), 200 (wide); Co 32 (single block), 36 (ragged mod 4 -> 64),
# 68 (ragged mod 64), 96 (the 32-remainder block), 128 (two full blocks)
BATCH = 2
WIDE = [(32, 32, 1, 1), (40, 36, 8, 16), (72, 68, 17, 33), (200, 96, 13, 49), (32, 128, 17, 33)]
# F(2x2) as a layer's own kernel (16 <= Co < 32, or Co no multiple of 4) and, Co > 32, split into 32-output blocks; 272 > 264: the 'W2+' bar
F2X2 = [(32, 24, 1, 1), (40, 34, 8, 16), (72, 68, 17, 33), (200, 96, 13, 49), (32, 128, 17, 33), (272, 70, 8, 16)]
STRIDE2 = [(32, 32, 1, 1), (40, 64, 9, 33), (72, 96, 18, 64), (200, 128, 9, 33)]          # Co multiples of 32: what b2f_s2b.hip packs
STRIDE2_RAGGED = [(40, 36, 9, 33)]                                                          # D2, E2 only
SMALL = [(5, 7, 8, 16), (40, 12, 17, 33), (72, 8, 1, 1)]                                    # Co < 16: the direct kernel at stride 1
FIXED = {"C16": [(16, 16, 1, 1), (16, 16, 17, 33)], "S16": [(16, 32, 1, 1), (16, 32, 9, 33), (16, 32, 18, 64)], "N2": [(32, 2, 1, 1), (32, 2, 17, 33)]}
FIRST = [(3, 16, 2, 2), (3, 16, 18, 66), (3, 16, 18, 64)]         # conv_first_kernel: even maps only (it computes H / 2 x W / 2): outputs 1 x 1, 9 x 33, 9 x 32
HEAD = [(1, 1), (9, 33), (18, 64)]                                                          # H, W of the head's 16-channel input

# the shapes each algorithm's emulation runs (the reference ratios): (Ci, Co, H, W, stride)
EMULATED = {
    "direct": [s + (1,) for s in SMALL + FIXED["C16"] + FIXED["N2"] + WIDE] + [s + (2,) for s in STRIDE2 + STRIDE2_RAGGED + FIXED["S16"] + FIRST],
    "direct-b": [s + (1,) for s in SMALL] + [s + (2,) for s in STRIDE2 + STRIDE2_RAGGED + FIRST],  # conv3x3_mfma's shapes (D1, D2) and the first layer's
    "F2": [s + (1,) for s in F2X2], "F4": [s + (1,) for s in WIDE], "F6": [s + (1,) for s in WIDE], "1D": [s + (1,) for s in WIDE],
}
EMU_TAG = {"direct": "D1", "direct-b": "D1", "F2": "W2", "F4": "W4", "F6": "W6"}      # the fp32 kernel whose bound the emulation of an algorithm must meet
SEED = 20

# ---- tile geometry: the sweep of tests/test_gpu_conv_edges.py -------------------------------------------------------------------------------
# id (CONFIGS of tests/test_gpu_conv_float64.py, 'HEAD', 'F1') -> (th, tw, bh, bw, where it is read), in OUTPUT pixels.  (th, tw): the tile --
# the Winograd tile, or the finest unit the kernel's inner loop cuts a block into, 1 where it has none; (bh, bw): what one block or work item
# computes.  UPDATE THIS TABLE when a kernel's tile or footprint changes: the sweep is generated from it.
GEOMETRY = {
    # conv3x3_mfma: at these sizes the four-wave forms, 4 x 32 or 8 x 16, whichever pads the map less: unit = what both cut, footprint = their hull
    "D1": (4, 16, 8, 32, "b2f_conv.hip:42,339-358"), "D2": (4, 16, 8, 32, "b2f_conv.hip:42,339-358"),
    "N2": (1, 1, 16, 16, "b2f_glue.hip:328,342"),
    "C16": (1, 16, 16, 32, "b2f_conv16.hip:6-7,30"),                 # 16-pixel M tiles of a row
    "S16": (1, 16, 4, 32, "b2f_conv16.hip:197-201,210"),
    "W2": (2, 2, 8, 16, "b2f_wino.hip:29,50"),
    "W4": (4, 4, 16, 32, "b2f_wino4.hip:19,76"),
    "W6": (6, 6, 12, 48, "b2f_wino6.hip:20,46"),
    "V1-1": (1, 4, 16, 32, "b2f_w1b.hip:16,25,55"), "V1-2": (1, 4, 16, 32, "b2f_w1b.hip:16,25,55"),      # F(4,3) along x: tiles of 4 columns
    "E1": (2, 1, 8, 32, "b2f_convb.hip:12,35"), "E1-direct": (2, 1, 8, 32, "b2f_convb.hip:12,35"),       # a wave owns rows 2 w, 2 w + 1
    "E2": (2, 1, 8, 32, "b2f_convb.hip:12,35"),
    "L2": (2, 1, 8, 16, "b2f_s2b.hip:9,13,31"),                      # pixel tiles of 2 rows x 16 columns
    "HEAD": (1, 16, 16, 30, "b2f_head.hip:8,15,36,299-303"),         # strips of 30 columns in 16-column tiles, cut into row blocks above 16 rows
    "F1": (1, 1, 8, 32, "b2f_glue.hip:226-227,233"),
    # experiments build (tools/experiments/csrc); a last n-block of <= 32 outputs of the three split forms is W4's
    "W4S": (4, 4, 16, 32, "b2f_wino4s.hip:28,50"), "W4H": (4, 4, 16, 32, "b2f_wino4.hip:19,76"),
    "W2S": (2, 2, 16, 16, "b2f_wino2s.hip:15,46"), "B16": (1, 16, 16, 32, "b2f_conv16b.hip:28"),
}
# (Ci, Co) per id: the smallest counts that run the kernel in each of its block forms (choose_kernel, csrc/b2f_api.hip, and the launchers)
_WIDE_CH = [(32, 64), (32, 32), (32, 96)]          # a 64-output n-block; the 32-output form; one launch holding both.  Ci 32: wino6's four chunks
EDGE_CHANNELS = {
    "D1": [(5, 7), (8, 12)],                                         # Co < 16, one N tile: scalar and 16-byte stores (b2f_conv.hip:121)
    "D2": [(8, 32), (8, 36), (8, 96), (8, 160)],                     # N tiles per block 1, 2 (ragged), 3, 4 x two n-blocks (conv_choose_tiles)
    "N2": [(8, 2), (40, 2)],                                         # two chunks per pass; four per pass, twice, the second partly (b2f_glue.hip:414)
    "C16": [(16, 16)], "S16": [(16, 32)], "B16": [(16, 16)],
    "W2": [(16, 24), (16, 70), (16, 64)],                            # one N tile; a two-tile block + a one-tile remainder; split into 32-output blocks
    "W4": _WIDE_CH, "W6": _WIDE_CH, "V1-1": _WIDE_CH, "V1-2": _WIDE_CH, "E1": _WIDE_CH, "W4S": _WIDE_CH, "W4H": _WIDE_CH, "W2S": _WIDE_CH,
    "E1-direct": [(5, 8), (8, 12)],
    "E2": [(16, 36), (16, 64), (16, 96)],                            # the one-tile kernel alone; the two-tile kernel; both (b2f_convb.hip:288-291)
    "L2": [(32, 32), (32, 64), (32, 160)],                           # 1, 2 and 5 output tiles of 32: one launch per four (b2f_s2b.hip:359-370)
    "HEAD": [(16, 32)], "F1": [(3, 16)],
}
EDGE_FAMILIES = ("gauss", "dc", "integers")


def edge_sizes(t, b):
    """every residue of the tile (1 .. t + 1), one under / on / one over the footprint, over two footprints, every multiple of 8 below it"""
    return sorted(s for s in set(range(1, t + 2)) | {b - 1, b, b + 1, 2 * b + 1} | set(range(8, b, 8)) if s > 0)


def edge_shapes(th, tw, bh, bw):
    """OUTPUT sizes (h, w) of the sweep: every height at one column over the footprint, every width at one row over it, and the small corners"""
    shapes = {(h, bw + 1) for h in edge_sizes(th, bh)} | {(bh + 1, w) for w in edge_sizes(tw, bw)}
    shapes |= {(h, w) for h in (1, th - 1, th + 1) for w in (1, tw - 1, tw + 1)}
    return sorted(s for s in shapes if s[0] > 0 and s[1] > 0)


def edge_inputs(cid, stride):
    """[(input H, input W, output h, output w)] of an id's sweep.  Stride 2: both input sizes that give an output size, 2 h - 1 and 2 h (the
    odd one reads the padding on the right / below, the even one does not); the first layer serves even maps only; the head's sizes are those
    of its stride-2 output"""
    out = []
    for h, w in edge_shapes(*GEOMETRY[cid][:4]):
        if stride == 1 and cid != "HEAD":
            out.append((h, w, h, w))
        else:
            out += [(2 * h - d, 2 * w - d, h, w) for d in ((0,) if cid == "F1" else (1, 0))]
    return out


def mutation_tile(cid):
    """the (th, tw) EDGE_MUTATIONS cut for an id: its tile, the footprint in a dimension where the tile is a single pixel"""
    th, tw, bh, bw = GEOMETRY[cid][:4]
    return (th if th > 1 else bh, tw if tw > 1 else bw)


def border_mask(h, w, th, tw):
    """h x w bool: the pixels whose tile is ragged or touches the map's edge (the first and last tile row and column)"""
    ty, tx = np.arange(h) // th, np.arange(w) // tw
    return ((ty == 0) | (ty == ty[-1]))[:, None] | ((tx == 0) | (tx == tx[-1]))[None, :]


def edge_case(family, ci, co, H, W, stride):
    """(x, w, b, conv64 with LeakyReLU, S_direct) of a sweep shape; not cached: the sweep holds thousands"""
    x, w, b = make_case(family, SEED, BATCH, ci, co, H, W)
    return x, w, b, conv64(x, w, b, stride, True), S_direct(x, w, b, stride)


@functools.lru_cache(maxsize=None)
def edge_emulation_case(alg, family, ci, co, H, W, stride, mutate=None, tile=None):
    """the float32 emulation of an algorithm on a sweep shape: (worst err / (u S of the algorithm), bit-exact against the float64 value --
    meaningful on `integers` only)"""
    x, w, b, val, Sd = edge_case(family, ci, co, H, W, stride)
    got = emulate(alg, x, w, b, stride, True, mutate, tile)
    S = Sd if alg in ("direct", "direct-b") else S_wino(x, w, b, alg)
    return measure(got, val, S)[0], bool(np.array_equal(got, round32_leaky(conv64(x, w, b, stride, False), True)))


def measure(got, val, S):
    """(worst |got - val| / (u S) over S > 0, its mean, worst |got - val|); a NaN in got gives an infinite ratio"""
    err = np.abs(np.asarray(got, np.float64) - val)
    err = np.where(np.isfinite(err), err, np.inf)
    pos = S > 0
    if not pos.any():
        return 0.0, 0.0, float(err.max())
    q = err[pos] / (U * S[pos])
    return float(q.max()), float(q.mean()), float(err.max())


@functools.lru_cache(maxsize=None)
def reference(family, shape, stride=1, leaky=True):
    """(x, w, b, conv64, S_direct) of a family at a shape, computed once and shared (do not write into them)"""
    Ci, Co, H, W = shape
    x, w, b = make_case(family, SEED, BATCH, Ci, Co, H, W)
    out = (x, w, b, conv64(x, w, b, stride, leaky), S_direct(x, w, b, stride))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wino_yardstick(family, shape, alg):
    x, w, b = reference(family, shape)[:3]
    s = S_wino(x, w, b, alg)
    s.setflags(write=False)
    return s


def emulation_n(alg, ci_padded):
    """n of the float32 emulation of an algorithm: the fp32 kernel's count"""
    if alg == "1D":
        return 3 * ci_padded + 8              # the fp32 form of b2f_w1b.hip's algorithm: 3 Ci products, the roundings of ROUNDINGS['V1']
    return n_roundings(EMU_TAG[alg], ci_padded)


def emulation_case(alg, family, shape, stride, mutate=None):
    """One emulation run: (worst err / (u S_direct), worst err / (u S of the algorithm), n of the fp32 kernel, exact zeros hold)"""
    x, w, b, val, Sd = reference(family, shape, stride)
    got = emulate(alg, x, w, b, stride, True, mutate)
    Sa = Sd if alg in ("direct", "direct-b") else wino_yardstick(family, shape, alg)
    return measure(got, val, Sd)[0], measure(got, val, Sa)[0], emulation_n(alg, padded(shape[0]))


def head_case(family, H, W):
    """(x, w1, b1, w2, b2) of the fused head.  integers: the first bias is raised by 576 >= max |sum|, so the hidden map is positive, a multiple
    of 2^-3 below 2^11 (h + m of the split hold it), and every later sum stays exact."""
    x, w1, b1 = make_case(family, SEED, BATCH, 16, 16, H, W)
    _, w2, b2 = make_case(family, SEED + 1, BATCH, 16, 32, H, W)
    if family == "integers":
        b1 = (b1 + f32(576)).astype(f32)
    return x, w1, b1, w2, b2


def head_measure(got, x, w1, b1, w2, b2):
    """(worst err / (u S2), its mean, worst err / head64's bound, worst |err|): S2 = the second layer's S_direct on the float64 map"""
    val, bnd = head64(x, w1, b1, w2, b2)
    S2 = S_direct(conv64(x, w1, b1, 1, True), w2, b2, 2)
    r, mean, worst = measure(got, val, S2)
    return r, mean, measure(got, val, bnd / U)[0], worst


def head_emulation_case(family, H, W):
    """two chained float32 direct convolutions, the head's emulation: (worst err / (u S2), worst err / bound)"""
    x, w1, b1, w2, b2 = head_case(family, H, W)
    r, _, rb, _ = head_measure(direct32(direct32(x, w1, b1, 1, True), w2, b2, 2, True), x, w1, b1, w2, b2)
    return r, rb


CN_MEAN = np.array([0.485, 0.456, 0.406], f32)          # ColorNormalize's constants as the kernel holds them (b2f_internal.h:184-185)
CN_STD = np.array([0.229, 0.224, 0.225], f32)


def first_case(family, shape, normalize):
    """The first layer on three frames, one draw of the family per frame: (x9: B x 9 x H x W for ops.conv_first, w, b, the float64 input of the
    reference: 3 B x 3 x H x W, image f * B + b, normalised in float64 with the float32 constants when normalize)"""
    _, _, H, W = shape
    frames = [make_case(family, SEED + f, BATCH, 3, 16, H, W) for f in range(3)]
    x64 = np.concatenate([fr[0] for fr in frames], 0).astype(np.float64)
    if normalize:
        x64 = (x64 - CN_MEAN.astype(np.float64)[None, :, None, None]) / CN_STD.astype(np.float64)[None, :, None, None]
    return np.concatenate([fr[0] for fr in frames], 1), frames[0][1], frames[0][2], x64


def first_norm_emulation_case(family, shape):
    """The normalised first layer in float32: x + (-mean) and the IEEE quotient, one rounding each, then the chain from the bias:
    (worst err / (u S_direct), n).  With ColorNormalize no family keeps integer inputs, so these ratios are recorded apart ('first-norm')."""
    x9, w, b, x64 = first_case(family, shape, True)
    B = x9.shape[0]
    x32 = np.concatenate([x9[:, 3 * f:3 * f + 3] for f in range(3)], 0)
    xn = ((x32 + (-CN_MEAN)[None, :, None, None]).astype(f32) / CN_STD[None, :, None, None]).astype(f32)
    got = direct32(xn, w, b, 2, True, None, True)
    return measure(got, conv64(x64, w, b, 2, True), S_direct(x64, w, b, 2))[0], n_roundings("F1", 3)


def compute_ratios():
    """{algorithm: {family: [worst err / (u S_direct), worst err / (u S of the algorithm)]}} of the float32 emulation over EMULATED[algorithm];
    'head': [worst err / (u S2), the same] over HEAD"""
    out = {}
    for alg in ALGS:
        out[alg] = {}
        for fam in FAMILIES:
            cases = [emulation_case(alg, fam, s[:4], s[4]) for s in EMULATED[alg]]
            out[alg][fam] = [max(c[0] for c in cases), max(c[1] for c in cases)]
    out["first-norm"] = {fam: [max(first_norm_emulation_case(fam, sh)[0] for sh in FIRST)] * 2 for fam in FAMILIES}
    out["head"] = {fam: [max(head_emulation_case(fam, H, W)[0] for H, W in HEAD)] * 2 for fam in FAMILIES}
    return out


@functools.lru_cache(maxsize=None)
def recorded_ratios():
    """tests/golden/conv_float64_ratios.json: compute_ratios() as recorded by `python -m tests.conv_float64`; tests/test_conv_float64_cpu.py
    holds the file to a fresh computation, the GPU file reads it"""
    with open(RATIOS_PATH) as f:
        return json.load(f)


def recorded(alg, family, own=False):
    """the emulation's worst err / (u S_direct) -- own: err / (u S of the algorithm itself) -- on a family"""
    return recorded_ratios()[alg][family][1 if own else 0]


# conv3x3_mfma (D1, D2) and the first layer start the chain at the bias.  A chain's rounding error has variance ~ u^2 sum_k p_k^2 over its
# partial sums p_k.  Bias last: p_k^2 ~ (k / N) s^2 (s: the deviation of the sum), sum = N s^2 / 2.  Bias first: p_k^2 ~ b^2 + (k / N) s^2,
# sum = N (b^2 + s^2 / 2): sqrt(1 + 2 b^2 / s^2) times the error, sqrt(3) for the tests' b ~ N(0, 1) on unit-variance sums.  These tags are
# held to 2 x their own emulation (direct-b) AND to 2 sqrt(3) x the plain bias-last emulation.
BIAS_FIRST_FACTOR = 3.0 ** 0.5


if __name__ == "__main__":
    with open(RATIOS_PATH, "w") as f:
        json.dump(compute_ratios(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(RATIOS_PATH).read())
