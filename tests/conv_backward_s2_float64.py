"""A float64 restatement of the backward pass of a stride-2 conv layer (nn.SpatialConvolution(Ci, Co, 3, 3, 2, 2, 1, 1) [+ LeakyReLU(0.2)]
:backward, pwc.lua:58-65, the first conv of a convUnit), its yardsticks, float32 emulations of the two kernels' summation orders, the bounds,
and the inputs and shapes of tests/test_conv_backward_s2_cpu.py and tests/test_gpu_conv_backward_s2.py.  Helper, no test; numpy / torch on the
CPU only.  tests/conv_float64.py supplies the families, u and measure(); tests/conv_backward_float64.py g' (masked64 / masked32) and bound_gw.

Definition (x: B x Ci x H x W, w: Co x Ci x 3 x 3, y and gy: B x Co x Ho x Wo, Ho = (H - 1) // 2 + 1, Wo = (W - 1) // 2 + 1):
    g'  = gy * (y > 0 ? 1 : 0.2) with the activation (y == 0 takes the slope), else gy
    gx[b, ci, iy, ix]   = sum over (co, ky, kx) with iy + 1 - ky and ix + 1 - kx even, oy = (iy + 1 - ky) / 2 in [0, Ho) and
                          ox = (ix + 1 - kx) / 2 in [0, Wo), of g'[b, co, oy, ox] w[co, ci, ky, kx]
    gw[co, ci, ky, kx]  = sum over (b, oy, ox) of g'[b, co, oy, ox] x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1], zero outside the map
    gb[co]              = sum over (b, oy, ox) of g'[b, co, oy, ox]
S_gx, S_gw, S_gb: the same sums on absolute values.

Bounds, u = 2^-24, first order; ROUNDINGS below cites the source lines.
    gw, gb: (longest_chain + partials + 2) u S, the stride-1 argument unchanged: the chain is the partial's in-map OUTPUT pixels.
    gx: (taps(py, px) * padded(Co) + 2) u S_gx elementwise, taps = 1, 2, 2, 4 by the parity class (iy & 1, ix & 1) of the pixel: one
    rounding per product the kernel's fmaf chain adds (the channels past Co are exact zeros), one for g', one spare.  The kernel adds no
    partial tiles: one accumulator holds an element's whole sum over co."""
import functools
import json
import os
import re

import numpy as np

from tests import conv_backward_float64 as K1
from tests import conv_float64 as F

U, f32, BATCH, SEED = F.U, F.f32, F.BATCH, F.SEED
RATIOS_PATH = os.path.join(F.ROOT, "tests", "golden", "conv_backward_s2_ratios.json")
KERNEL_SOURCE = K1.KERNEL_SOURCE

# what each term of the bounds counts, and where back2future_amd/csrc/b2f_convbwd.hip does it
ROUNDINGS = {
    "g'": "b2f_convbwd.hip:116 leaky_mask: g[j] = v[j] > 0.f ? g[j] : 0.2f * g[j] -- one rounding of 0.2f * gy (0.2f is 0.25 u from 0.2)",
    "gw chain": "b2f_convbwd.hip:213 conv3x3_gradw<MC, NC, 2>: acc[tap] = mfma_f32_32x32x2f32(a, b[tap], acc[tap]) over the strips s0 .. s1 of a partial -- "
                "one fmaf per in-map output pixel (the masked loads stage zeros elsewhere), at most longest_chain of the plan query",
    "gw partials": "b2f_convbwd.hip:277, :282 gradw_reduce: a = a + src[k * plane], k = 1 .. P - 1 in index order -- P - 1 roundings, counted as P",
    "gx chain": "b2f_convbwd.hip:374-382 conv3x3s2_gradx: acc[class] = mfma_f32_32x32x2f32(a[tap], b.., acc[class]) for k = 0 .. co_pad in steps of 2 -- taps(class) "
                "fmafs per output channel, 1 / 2 / 2 / 4 for class (0,0) / (0,1) / (1,0) / (1,1); channels past Co multiply staged zeros",
    "spare": "one for the store path of either kernel",
}

# parity class (py, px) -> its taps in the kernel's order: (ky, kx, dy, dx), the tap reads g'[oy + dy, ox + dx]
CLASS_TAPS = {
    (0, 0): [(1, 1, 0, 0)],
    (0, 1): [(1, 0, 0, 1), (1, 2, 0, 0)],
    (1, 0): [(0, 1, 1, 0), (2, 1, 0, 0)],
    (1, 1): [(0, 0, 1, 1), (0, 2, 1, 0), (2, 0, 0, 1), (2, 2, 0, 0)],
}


def out_size(n):
    return (n - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """{name: value} of the constexpr ints csrc/b2f_convbwd.hip names in its header: kGradwBandRows, kGradwS2StripCols, kGradxS2Rows, ..."""
    with open(KERNEL_SOURCE) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kGrad[wx]\w+) = (\d+);", f.read())}


def edge_maps():
    """(H, W) of the input: output sizes one under, on and one over the gradw kernel's strip and the gradx kernel's tile in each dimension,
    each at both input sizes 2 h - 1 and 2 h that give it"""
    k = kernel_constants()
    maps = []
    for rows, cols in ((k["kGradwBandRows"], k["kGradwS2StripCols"]), (k["kGradxS2Rows"], k["kGradxS2Cols"])):
        for d in (-1, 0, 1):
            h, w = max(rows + d, 1), cols + d
            maps += [(2 * h - 1, 2 * w - 1), (2 * h, 2 * w)]
    return maps


# (Ci, Co, H, W) of the input, batch 2: the centre tap alone; a 1 x 1 output from a 2 x 2 input; ragged Ci and Co; the first layer at an
# even and an odd map; the six pyramid widths.  Then the edge maps on channel counts that run the block forms of conv3x3_gradw the list
# leaves out (1 x 2 and 3 x 1 tiles of 32 channels) and a ragged multi-tile one.
SHAPES = [(32, 32, 1, 1), (32, 32, 2, 2), (5, 7, 8, 16), (3, 16, 18, 66), (3, 16, 17, 33), (16, 32, 9, 33), (16, 32, 18, 64), (40, 36, 17, 34),
          (64, 96, 13, 49), (96, 128, 8, 16), (128, 192, 5, 7)]
EDGE_CHANNELS = [(64, 8), (32, 96), (40, 36)]
FORCED = [(40, 36, 17, 34), (64, 96, 13, 49)]          # op_gradw_partials = 3: 20 strips as 7 + 7 + 6, 16 strips as 6 + 6 + 4
MUTATION_SHAPE = (32, 32, 9, 17)                       # Ci == Co, so that w transposed still has a shape; odd H and W
GX_MUTATIONS = ("swap-parity", "drop-halo-row", "write-last-odd-row", "mask-from-gy", "w-transposed")
GW_MUTATIONS = ("x-shift", "mask-from-gy")


def all_shapes():
    maps = edge_maps()
    return SHAPES + [EDGE_CHANNELS[i % len(EDGE_CHANNELS)] + m for i, m in enumerate(maps)]


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------

def _sums(x, w, g):
    """(gx, gw, gb) of the definition in float64 from g', with explicit loops over the taps"""
    x, w, g = (np.asarray(a, np.float64) for a in (x, w, g))
    B, Ci, H, W = x.shape
    Ho, Wo = g.shape[2:]
    assert (Ho, Wo) == (out_size(H), out_size(W))
    xp = np.zeros((B, Ci, 2 * Ho + 2, 2 * Wo + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    gxp = np.zeros_like(xp)             # gx with one pixel of padding: index iy + 1
    gw = np.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            rows, cols = slice(ky, ky + 2 * Ho, 2), slice(kx, kx + 2 * Wo, 2)          # iy + 1 = 2 oy + ky
            gxp[:, :, rows, cols] += np.einsum("bohw,oc->bchw", g, w[:, :, ky, kx], optimize=True)
            gw[:, :, ky, kx] = np.einsum("bohw,bchw->oc", g, xp[:, :, rows, cols], optimize=True)
    return np.ascontiguousarray(gxp[:, :, 1:H + 1, 1:W + 1]), gw, g.sum((0, 2, 3))


def backward64(x, w, y, gy, leaky):
    return _sums(x, w, K1.masked64(gy, y, leaky))


def yardsticks(x, w, y, gy, leaky):
    """(S_gx, S_gw, S_gb)"""
    return _sums(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(K1.masked64(gy, y, leaky)))


# ---- float32 emulations ----------------------------------------------------------------------------------------------------------------

def gradw32(x, g, partials, stride=2, mutate=None):
    """(gw, gb) in float32 as the split computes them, for a layer of this stride: the OUTPUT pixels (b, oy, ox) in that order are cut into
    `partials` runs of ceil(pixels / partials); a run is a chain in pixel order, product and sum each rounded; the runs are added in index
    order.  mutate 'x-shift': x is read at stride * oy + ky instead of stride * oy + ky - 1."""
    x, g = np.asarray(x, f32), np.asarray(g, f32)
    B, Ci, H, W = x.shape
    Co, Ho, Wo = g.shape[1:]
    off = 0 if mutate == "x-shift" else 1
    xp = np.zeros((B, Ci, stride * Ho + 3, stride * Wo + 3), f32)
    xp[:, :, off:off + H, off:off + W] = x
    n = B * Ho * Wo
    q = -(-n // partials)
    total_w = total_b = None
    for p0 in range(0, n, q):
        acc_w, acc_b = np.zeros((Co, Ci, 3, 3), f32), np.zeros(Co, f32)
        for i in range(p0, min(p0 + q, n)):
            b, oy, ox = i // (Ho * Wo), (i // Wo) % Ho, i % Wo
            gv = g[b, :, oy, ox]
            acc_w = acc_w + gv[:, None, None, None] * xp[b, :, stride * oy:stride * oy + 3, stride * ox:stride * ox + 3][None]
            acc_b = acc_b + gv
        total_w, total_b = (acc_w, acc_b) if total_w is None else (total_w + acc_w, total_b + acc_b)
    assert total_w.dtype == f32 and total_b.dtype == f32
    return total_w, total_b


def gradx_s2_32(g, w, H, W, mutate=None):
    """gx in float32 in conv3x3s2_gradx's order: per parity class one chain over (pair of output channels, tap of the class in CLASS_TAPS'
    order, channel of the pair), product and sum each rounded; g' is zero in the halo row and column past the map.
    mutate: 'swap-parity' rows of parity py take the taps of parity 1 - py; 'drop-halo-row' the row oy + 1 reads zero; 'write-last-odd-row'
    at odd H the row H, which does not exist, is stored where it lands in memory, on row 0 of the next image; 'w-transposed' w[ci][co]."""
    g, w = np.asarray(g, f32), np.asarray(w, f32)
    if mutate == "w-transposed":
        w = np.ascontiguousarray(w.transpose(1, 0, 2, 3))
    B, Co, Ho, Wo = g.shape
    Ci = w.shape[1]
    gp = np.zeros((B, Co + (Co & 1), Ho + 1, Wo + 1), f32)
    gp[:, :Co, :Ho, :Wo] = g
    wp = np.zeros((Co + (Co & 1), Ci, 3, 3), f32)
    wp[:Co] = w
    gx = np.zeros((B, Ci, H, W), f32)
    for (py, px), taps in CLASS_TAPS.items():
        if mutate == "swap-parity":
            taps = CLASS_TAPS[(1 - py, px)]
        acc = np.zeros((B, Ci, Ho, Wo), f32)
        for co in range(0, gp.shape[1], 2):
            for ky, kx, dy, dx in taps:
                for k in (co, co + 1):
                    src = gp[:, k, dy:dy + Ho, dx:dx + Wo]
                    if mutate == "drop-halo-row" and dy == 1:
                        src = np.zeros_like(src)
                    acc = acc + src[:, None] * wp[k, :, ky, kx][None, :, None, None]          # float32 * float32, then float32 + float32
        assert acc.dtype == f32
        rows, cols = len(range(py, H, 2)), len(range(px, W, 2))
        gx[:, :, py::2, px::2] = acc[:, :, :rows, :cols]
        if mutate == "write-last-odd-row" and py == 1 and H % 2 == 1:
            gx[1:, :, 0, px::2] = acc[:-1, :, Ho - 1, :cols]
    return gx


def emulated_chain(B, Ho, Wo, partials):
    """(partials, longest chain) of gradw32's split"""
    return K1.emulated_chain(B, Ho, Wo, partials)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------

bound_gw = K1.bound_gw


def gx_roundings(co, H, W):
    """n of gx's bound n u S_gx, H x W: taps(py, px) * padded(Co) + 2"""
    taps = np.zeros((H, W))
    for (py, px), t in CLASS_TAPS.items():
        taps[py::2, px::2] = len(t)
    return taps * F.padded(co) + 2


def bound_gx(co, S):
    return gx_roundings(co, S.shape[2], S.shape[3])[None, None] * U * S


def measure_gx(got, val, S, co):
    """the worst (err / (u S_gx), err / bound)"""
    n = np.broadcast_to(gx_roundings(co, S.shape[2], S.shape[3])[None, None], S.shape)
    return F.measure(got, val, S)[0], F.measure(got, val, S * n)[0]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(family, shape, leaky):
    """(x, w, y, gy) float32, computed once and shared (read-only): x, w of make_case; gy of the same family's generator with another
    seed on the output map; y = conv64(x, w, b, 2, leaky) rounded to float32 with 3 % of its elements exactly 0 (None without the activation)"""
    Ci, Co, H, W = shape
    x, w, b = F.make_case(family, SEED, BATCH, Ci, Co, H, W)
    gy = F.make_case(family, SEED + 1, BATCH, Co, Ci, out_size(H), out_size(W))[0]
    y = None
    if leaky:
        y = F.conv64(x, w, b, 2, True).astype(f32)
        y[np.random.default_rng([SEED + 2, F.FAMILIES.index(family), Ci, Co, H, W]).random(y.shape) < 0.03] = 0
    out = (x, w, y, gy)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(family, shape, leaky):
    """((gx, gw, gb) of backward64, (S_gx, S_gw, S_gb), g' in float64), computed once and shared (read-only)"""
    x, w, y, gy = case(family, shape, leaky)
    g = K1.masked64(gy, y, leaky)
    out = (_sums(x, w, g), _sums(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), np.abs(g)), g)
    for a in out[0] + out[1] + (g,):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gradw_emulation_case(family, shape, partials, mutate=None):
    """gradw32 at stride 2 with the activation on a case: (worst err / (u S_gw), worst err / bound_gw, the same two for gb)"""
    x, w, y, gy = case(family, shape, True)
    (_, gw, gb), (_, Sw, Sb), _ = reference(family, shape, True)
    got_w, got_b = gradw32(x, K1.masked32(gy, y, True, mutate), partials, 2, mutate)
    P, chain = emulated_chain(BATCH, out_size(shape[2]), out_size(shape[3]), partials)
    n = chain + P + 2
    rw, rb = F.measure(got_w, gw, Sw)[0], F.measure(got_b, gb, Sb)[0]
    return rw, rw / n, rb, rb / n


@functools.lru_cache(maxsize=None)
def gradx_emulation_case(family, shape, mutate=None):
    """gradx_s2_32 with the activation on a case: (worst err / (u S_gx), worst err / bound_gx)"""
    x, w, y, gy = case(family, shape, True)
    (gx, _, _), (Sx, _, _), _ = reference(family, shape, True)
    got = gradx_s2_32(K1.masked32(gy, y, True, mutate), w, shape[2], shape[3], mutate)
    return measure_gx(got, gx, Sx, shape[1])


def compute_ratios():
    """{"gw": {family: worst err / (u S_gw) of gradw32 over all_shapes() and partials 1 and 3}, "gx": {family: the same of gradx_s2_32}}"""
    return {"gw": {fam: max(gradw_emulation_case(fam, s, P)[0] for s in all_shapes() for P in (1, 3)) for fam in F.FAMILIES},
            "gx": {fam: max(gradx_emulation_case(fam, s)[0] for s in all_shapes()) for fam in F.FAMILIES}}


@functools.lru_cache(maxsize=None)
def recorded_ratios():
    """tests/golden/conv_backward_s2_ratios.json: compute_ratios() as recorded by `python -m tests.conv_backward_s2_float64`;
    tests/test_conv_backward_s2_cpu.py holds the file to a fresh computation, the GPU file reads it"""
    with open(RATIOS_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(RATIOS_PATH, "w") as f:
        json.dump(compute_ratios(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(RATIOS_PATH).read())
