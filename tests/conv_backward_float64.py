"""A float64 restatement of the backward pass of a stride-1 conv layer (nn.SpatialConvolution(Ci, Co, 3, 3, 1, 1, 1, 1) [+ LeakyReLU(0.2)]
:backward, pwc.lua:58-65,76-85), its yardsticks, a float32 emulation of the gradWeight kernel's split sum, and the inputs and shapes of
tests/test_conv_backward_cpu.py and tests/test_gpu_conv_backward.py.  Helper, no test; numpy / torch on the CPU only.  The forward's
helper tests/conv_float64.py supplies the families, u, the forward kernels' bounds and yardsticks (gradInput runs on those kernels).

Definition (x: B x Ci x H x W, w: Co x Ci x 3 x 3, y: the layer's output, gy: the gradient with respect to y):
    g'  = gy * (y > 0 ? 1 : 0.2) with the activation (y == 0 takes the slope: nn.LeakyReLU:updateGradInput tests input > 0), else gy
    gx[b, ci, iy, ix]   = sum over (co, ky, kx) of g'[b, co, iy + 1 - ky, ix + 1 - kx] w[co, ci, ky, kx], zero outside the map
                        = conv3x3(g', w~, bias 0), w~[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx]
    gw[co, ci, ky, kx]  = sum over (b, oy, ox) of g'[b, co, oy, ox] x[b, ci, oy + ky - 1, ox + kx - 1], zero padding
    gb[co]              = sum over (b, oy, ox) of g'[b, co, oy, ox]
S_gx, S_gw, S_gb: the same sums on absolute values.

Bounds, u = 2^-24, first order.
    gw, gb: (longest_chain + partials + 2) u S.  csrc/b2f_convbwd.hip: conv3x3_gradw adds the pixels of a partial into an fp32 MFMA
    accumulator, an fmaf chain with one rounding per pixel (gradw32 below rounds the product and the sum: at least as many); padding
    pixels add an exact zero, so the chain is the partial's in-map pixels, at most longest_chain of the plan query; gradw_reduce adds the
    partials in index order, one rounding each (partials - 1, counted as partials); leaky_mask's 0.2f * gy is one rounding (0.2f itself is
    0.25 u from 0.2); one is spare for the store path.
    gx: bound(tag, padded(Co), S) + u S_direct(|g'|, |w~|): tag = the forward kernel that ran, S its own yardstick on (g', w~), the second
    term the rounding of g'."""
import functools
import json
import os
import re

import numpy as np

from tests import conv_float64 as F

U, f32, BATCH, SEED = F.U, F.f32, F.BATCH, F.SEED
RATIOS_PATH = os.path.join(F.ROOT, "tests", "golden", "conv_backward_ratios.json")
KERNEL_SOURCE = os.path.join(F.ROOT, "back2future_amd", "csrc", "b2f_convbwd.hip")


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """{name: value} of the constexpr ints csrc/b2f_convbwd.hip names in its header: kGradwBandRows, kGradwStripCols, ..."""
    with open(KERNEL_SOURCE) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kGradw\w+) = (\d+);", f.read())}


def edge_maps():
    """(H, W): one pixel under, on and one over the gradw kernel's row band and pixel strip, in each dimension"""
    k = kernel_constants()
    rb, sw = k["kGradwBandRows"], k["kGradwStripCols"]
    return [(max(rb - 1, 1), sw - 1), (rb, sw), (rb + 1, sw + 1)]


# (Ci, Co, H, W), batch 2: the centre tap alone; ragged Ci and Co; the last decoder layer (its gradInput conv has one input chunk); the
# forward sweep's wide shapes; a first decoder layer's width.  Then the edge maps, on channel counts that run the block forms of
# conv3x3_gradw the list above leaves out (1 x 2 and 3 x 2 tiles of 32 channels) and the four-wave one.
SHAPES = [(32, 32, 1, 1), (5, 7, 8, 16), (8, 2, 17, 33), (40, 36, 17, 33), (72, 68, 13, 49), (200, 96, 13, 49), (32, 128, 17, 33),
          (196, 128, 8, 16)]
EDGE_CHANNELS = [(64, 8), (64, 96), (40, 36)]
FORCED = [(40, 36, 17, 33), (72, 68, 13, 49)]          # op_gradw_partials = 3: a ragged last partial
MUTATION_SHAPE = (32, 32, 8, 16)                       # Ci == Co, so that w~ without the transpose still has a shape
MUTATIONS = ("mask-from-gy", "no-rotation", "no-transpose", "drop-last-column", "partial-twice")


def all_shapes():
    return SHAPES + [c + m for c, m in zip(EDGE_CHANNELS, edge_maps())]


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------

def masked64(gy, y, leaky, mutate=None):
    """g' in float64"""
    gy = np.asarray(gy, np.float64)
    if not leaky:
        return gy
    sign = gy if mutate == "mask-from-gy" else np.asarray(y, np.float64)
    return np.where(sign > 0, gy, 0.2 * gy)


def rotated(w, mutate=None):
    """w~[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx]"""
    w = np.asarray(w)
    if mutate != "no-rotation":
        w = w[:, :, ::-1, ::-1]
    return np.ascontiguousarray(w if mutate == "no-transpose" else w.transpose(1, 0, 2, 3))


def _sums(x, w, g):
    """(gx, gw, gb) of the definition in float64 from g', with explicit loops over the taps"""
    x, w, g = (np.asarray(a, np.float64) for a in (x, w, g))
    B, Ci, H, W = x.shape
    xp = np.zeros((B, Ci, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    gp = np.zeros((B, g.shape[1], H + 2, W + 2))
    gp[:, :, 1:-1, 1:-1] = g
    gx, gw = np.zeros_like(x), np.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            gx += np.einsum("bohw,oc->bchw", gp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w[:, :, ky, kx], optimize=True)
            gw[:, :, ky, kx] = np.einsum("bohw,bchw->oc", g, xp[:, :, ky:ky + H, kx:kx + W], optimize=True)
    return gx, gw, g.sum((0, 2, 3))


def backward64(x, w, y, gy, leaky):
    return _sums(x, w, masked64(gy, y, leaky))


def yardsticks(x, w, y, gy, leaky):
    """(S_gx, S_gw, S_gb)"""
    return _sums(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(masked64(gy, y, leaky)))


# ---- float32 emulations ----------------------------------------------------------------------------------------------------------------

def masked32(gy, y, leaky, mutate=None):
    """g' as leaky_mask computes it: gy, or 0.2f * gy rounded once where y <= 0"""
    gy = np.asarray(gy, f32)
    if not leaky:
        return gy
    sign = gy if mutate == "mask-from-gy" else np.asarray(y, f32)
    return np.where(sign > 0, gy, (f32(0.2) * gy).astype(f32)).astype(f32)


def gradw32(x, g, partials, mutate=None):
    """(gw, gb) in float32 as the split computes them: the pixels (b, oy, ox) in that order are cut into `partials` runs of
    ceil(pixels / partials); a run is a chain in pixel order, product and sum each rounded; the runs are added in index order.
    mutate: 'drop-last-column' a run leaves out its pixels of the last column, 'partial-twice' run 0 is added twice."""
    x, g = np.asarray(x, f32), np.asarray(g, f32)
    B, Ci, H, W = x.shape
    Co = g.shape[1]
    xp = np.zeros((B, Ci, H + 2, W + 2), f32)
    xp[:, :, 1:-1, 1:-1] = x
    n = B * H * W
    q = -(-n // partials)
    total_w = total_b = None
    for p0 in range(0, n, q):
        acc_w, acc_b = np.zeros((Co, Ci, 3, 3), f32), np.zeros(Co, f32)
        for i in range(p0, min(p0 + q, n)):
            b, oy, ox = i // (H * W), (i // W) % H, i % W
            if mutate == "drop-last-column" and ox == W - 1:
                continue
            gv = g[b, :, oy, ox]
            acc_w = acc_w + gv[:, None, None, None] * xp[b, :, oy:oy + 3, ox:ox + 3][None]          # float32 * float32, then float32 + float32
            acc_b = acc_b + gv
        if total_w is None:
            total_w, total_b = acc_w, acc_b
            if mutate == "partial-twice":
                total_w, total_b = total_w + acc_w, total_b + acc_b
        else:
            total_w, total_b = total_w + acc_w, total_b + acc_b
    assert total_w.dtype == f32 and total_b.dtype == f32
    return total_w, total_b


def gradx32(g, w, mutate=None):
    """gx in float32 on the direct algorithm: conv3x3(g', w~, bias 0)"""
    wt = rotated(np.asarray(w, f32), mutate)
    return F.direct32(g, wt, np.zeros(wt.shape[0], f32), 1, False)


def emulated_chain(B, H, W, partials):
    """(partials, longest chain) of gradw32's split"""
    n = B * H * W
    q = -(-n // partials)
    return -(-n // q), min(q, n)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------

def bound_gw(longest_chain, partials, S):
    return (longest_chain + partials + 2) * U * S


def bound_gx(tag, co, S, S_rounding):
    """S: the yardstick of the forward kernel `tag` on (g', w~); S_rounding = S_direct(|g'|, |w~|)"""
    return F.bound(tag, F.padded(co), S) + U * S_rounding


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(family, shape, leaky):
    """(x, w, y, gy) float32, computed once and shared (read-only): x, w of make_case; gy of the same family's generator with another
    seed; y = conv64(x, w, b, 1, leaky) rounded to float32 with 3 % of its elements exactly 0 (None without the activation)"""
    Ci, Co, H, W = shape
    x, w, b = F.make_case(family, SEED, BATCH, Ci, Co, H, W)
    gy = F.make_case(family, SEED + 1, BATCH, Co, Ci, H, W)[0]
    y = None
    if leaky:
        y = F.conv64(x, w, b, 1, True).astype(f32)
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
    g = masked64(gy, y, leaky)
    out = (_sums(x, w, g), _sums(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), np.abs(g)), g)
    for a in out[0] + out[1] + (g,):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulation_case(family, shape, partials, mutate=None):
    """gradw32 with the activation on a case: (worst err / (u S_gw), worst err / bound_gw, the same two for gb)"""
    x, w, y, gy = case(family, shape, True)
    (_, gw, gb), (_, Sw, Sb), _ = reference(family, shape, True)
    got_w, got_b = gradw32(x, masked32(gy, y, True, mutate), partials, mutate)
    P, chain = emulated_chain(BATCH, shape[2], shape[3], partials)
    n = chain + P + 2
    rw, rb = F.measure(got_w, gw, Sw)[0], F.measure(got_b, gb, Sb)[0]
    return rw, rw / n, rb, rb / n


def gradx_mutation_case(family, shape, mutate):
    """gradx32 on a case against gx's bound on the direct kernel: worst err / bound"""
    x, w, y, gy = case(family, shape, True)
    (gx, _, _), _, g = reference(family, shape, True)
    wt = rotated(w.astype(np.float64))
    zero = np.zeros(wt.shape[0])
    S = F.S_direct(g, wt, zero)
    got = gradx32(masked32(gy, y, True, mutate if mutate == "mask-from-gy" else None), w, mutate)
    return F.measure(got, gx, bound_gx("D1", shape[1], S, S) / U)[0]


def compute_ratios():
    """{family: worst err / (u S_gw) of gradw32 over all_shapes() and partials 1 and 3}"""
    return {fam: max(emulation_case(fam, s, P)[0] for s in all_shapes() for P in (1, 3)) for fam in F.FAMILIES}


@functools.lru_cache(maxsize=None)
def recorded_ratios():
    """tests/golden/conv_backward_ratios.json: compute_ratios() as recorded by `python -m tests.conv_backward_float64`;
    tests/test_conv_backward_cpu.py holds the file to a fresh computation, the GPU file reads it"""
    with open(RATIOS_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(RATIOS_PATH, "w") as f:
        json.dump(compute_ratios(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(RATIOS_PATH).read())
