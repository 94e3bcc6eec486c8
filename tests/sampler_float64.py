"""Float64 restatement of nn.BilinearSamplerBHWD in its CUDA form (the reference's extras/stnbhwd/BilinearSamplerBHWD.cu: forward :41-115,
backward :161-307), the counted bounds it is held to, and the shapes and grids of tests/test_gpu_reference_sampler.py and
tests/test_reference_recipe_cpu.py.  Helper, no test; numpy on the CPU only.  Layouts are the module's: images B x h x w x C, grids
B x gh x gw x 2 with x first.  The grid sizes the output, the image sizes the clamp (BilinearSamplerBHWD.lua:26-41,70).

Coordinates are part of the specification, as in tests/glue_float64.py: c = grid + position, the clamp to [0, size - 1], the floor,
w = 1 - (c - floor c) and 1 - w are float32, one rounding each (getTopLeft, :6-20; glue_float64.top_left).  No correct implementation can
reassociate them, so the float64 side takes the cell and the four weights as given and computes everything after them in float64.

Bound per output: n * 2^-24 * S, S = the float64 sum of the absolute values of the terms, n = the float32 roundings on the longest path
of one output, counted from the reference's expressions (first order, as glue_float64.ROUNDINGS).  A contracted multiply-add rounds
once where the separate operations round twice, so the counts hold for a build with contraction as well.  Where S = 0 the result is 0.

  forward (:107-110)        v = xw * yw * tl + (1 - xw) * yw * tr + xw * (1 - yw) * bl + (1 - xw) * (1 - yw) * br
                            on tl's path: xw * yw 1, * tl 1, three additions 3                                          n = 5
                            S = sum over the four taps of |w_a w_b tap|
  grid gradient (:232-288)  a lane adds its m = ceil(C / 32) products in turn: the product 1, m - 1 additions (the first lands on the
                            zero the accumulator starts from: exact); the tree of sumReduceShMem (:27-36) has five levels 5; then
                            -xw * d 1 and three additions 3                                                             n = m + 9
                            S = sum over the four taps of |weight of :287-288| * sum_t |img_t * gradOutput_t|
  image gradient (:236-261) one scattered term is (w_a * w_b) * gradOutput: 2; an element that K terms land on is their sum in an
                            order the atomics choose: the first lands on the zero the buffer starts from, K - 1 additions follow
                                                                                                                        n = K + 1
                            S = sum of |w_a w_b gradOutput| over those K terms; K is counted by the float64 scatter, per element
A tap outside the image is skipped (:94-97, :221-224): it adds no term, no S and no K."""
import functools

import numpy as np

from tests import glue_float64 as GF

U = GF.U
f32, f64 = np.float32, np.float64
SEED = 29
B = 2
N_FORWARD = 5
LANES = 32           # threadIdx.x of the reference's 32 x 16 block: the stride of the per-lane sums
TREE_LEVELS = 5      # 16, 8, 4, 2, 1

# (C, image h, image w, grid h, grid w)
CASES = [
    (3, 1, 1, 1, 1),          # width - 1 = 0
    (1, 1, 16, 1, 16),        # one channel, exactly one 16-pixel block
    (32, 3, 17, 3, 17),       # one pixel past a block: the withinGridBounds tail
    (40, 7, 33, 7, 33),       # the strided partial sums wrap
    (33, 2, 48, 2, 48),       # the same wrap, by one channel
    (128, 6, 5, 6, 5),        # four channels per lane
    (8, 5, 9, 4, 20),         # the grid sizes the output, the image sizes the clamp
]
FIELDS = ("frac", "whole", "edges", "far")
UNIT_K = (-20.0, 20.0, 2.5)


def case_id(case):
    return "C%d-%dx%d-grid%dx%d" % case


def n_grid(C):
    """roundings on the longest path of one grid-gradient component: see the module's head"""
    m = -(-C // LANES)
    return 1 + (m - 1) + TREE_LEVELS + 1 + 3


def n_image(K):
    """roundings on the longest path of an image-gradient element that K terms are scattered into (0 where K = 0)"""
    K = np.asarray(K)
    return np.where(K > 0, K + 1, 0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def _rng(tag, case, *more):
    return np.random.default_rng([SEED, tag] + list(case) + list(more))


def image(case):
    C, ih, iw, gh, gw = case
    return _rng(1, case).standard_normal((B, ih, iw, C), dtype=f32)


def grad_output(case):
    C, ih, iw, gh, gw = case
    return _rng(2, case).standard_normal((B, gh, gw, C), dtype=f32)


# `edges`: what one axis of one pixel aims at, by the pixel's running index: the first column / row, the last, half a pixel beyond
# either, and two fractional draws, so that an edge on one axis meets a blend on the other.  36 pixels see every pair.
EDGE_CLASSES = 6


def _edge_axis(cls, pos, size, frac):
    target = np.select([cls == 0, cls == 1, cls == 2, cls == 3], [0.0, size - 1.0, -0.5, size - 0.5], default=np.nan)
    return np.where(cls >= 4, frac, target - pos)          # small half-integers: exact in float32


def grid(field, case):
    """B x gh x gw x 2 float32, finite: the displacement the sampler adds to the output pixel's own position.
    frac: N(0, 3 px).  whole: whole pixels -4 .. 4, every fourth zero a -0.0.  edges: see EDGE_CLASSES.  far: +-(max(h, w) + 5) on each
    axis, the four sign pairs in turn."""
    C, ih, iw, gh, gw = case
    r = _rng(3, case, FIELDS.index(field))
    shape = (B, gh, gw, 2)
    idx = np.arange(B * gh * gw).reshape(B, gh, gw)
    if field == "frac":
        g = r.standard_normal(shape) * 3.0
    elif field == "whole":
        g = r.integers(-4, 5, shape).astype(f64)
        flat = g.reshape(-1)
        zeros = np.flatnonzero(flat == 0)
        flat[zeros[::4]] = -0.0
        if flat.size and not np.signbit(flat).any():
            flat[0] = -0.0
    elif field == "edges":
        frac = r.standard_normal(shape) * 1.5
        xs = np.broadcast_to(np.arange(gw, dtype=f64)[None, None, :], idx.shape)
        ys = np.broadcast_to(np.arange(gh, dtype=f64)[None, :, None], idx.shape)
        g = np.stack([_edge_axis(idx % EDGE_CLASSES, xs, iw, frac[..., 0]),
                      _edge_axis((idx // EDGE_CLASSES) % EDGE_CLASSES, ys, ih, frac[..., 1])], -1)
    elif field == "far":
        d = float(max(ih, iw, gh, gw) + 5)
        g = np.stack([np.where(idx % 2 == 0, d, -d), np.where((idx // 2) % 2 == 0, d, -d)], -1)
    else:
        raise KeyError(field)
    g = g.astype(f32)
    assert g.shape == shape and np.isfinite(g).all()
    return g


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def _floor_first(c, size):
    """a wrong getTopLeft: the floor and the weight taken before the clamp, the clamp applied to the index"""
    fl = np.floor(c)
    return np.clip(fl, 0, size - 1).astype(np.int64), (f32(1) - (c - fl).astype(f32)).astype(f32)


def cells(grid_, ih, iw, mutate=None):
    """getTopLeft on both axes in float32: dict of xl, yt (int64), xw, yw, ux = 1 - xw, uy = 1 - yw (float32), x1, y1 (the right / lower
    neighbour is inside), xc, yc (the coordinate before the clamp), each B x gh x gw.  mutate, for tests/test_reference_recipe_cpu.py:
    'frac' (glue_float64.top_left's: the weights exchanged), 'floor-first', 'xy' (the grid read y first)"""
    assert grid_.dtype == f32
    _, gh, gw, _ = grid_.shape
    gx, gy = (grid_[..., 1], grid_[..., 0]) if mutate == "xy" else (grid_[..., 0], grid_[..., 1])
    xc = (gx + np.arange(gw, dtype=f32)[None, None, :]).astype(f32)
    yc = (gy + np.arange(gh, dtype=f32)[None, :, None]).astype(f32)
    if mutate == "floor-first":
        (xl, xw), (yt, yw) = _floor_first(xc, iw), _floor_first(yc, ih)
    else:
        xl, xw = GF.top_left(xc, iw, mutate if mutate == "frac" else None)
        yt, yw = GF.top_left(yc, ih, mutate if mutate == "frac" else None)
    return dict(xl=xl, yt=yt, xw=xw, yw=yw, ux=(f32(1) - xw).astype(f32), uy=(f32(1) - yw).astype(f32),
                x1=xl + 1 <= iw - 1, y1=yt + 1 <= ih - 1, xc=xc, yc=yc)


def _taps(c):
    """the four taps in the reference's order (tl, tr, bl, br): (dy, dx, inside, weight along x, weight along y), weights float64"""
    xw, yw, ux, uy = (c[k].astype(f64) for k in ("xw", "yw", "ux", "uy"))
    always = np.ones_like(c["x1"])
    return [(0, 0, always, xw, yw), (0, 1, c["x1"], ux, yw), (1, 0, c["y1"], xw, uy), (1, 1, c["x1"] & c["y1"], ux, uy)]


def _gather(img64, c, dy, dx, inside):
    """the tap's channels per output pixel, B x gh x gw x C; zeros where the tap is outside"""
    Bn, ih, iw, _ = img64.shape
    b = np.arange(Bn)[:, None, None]
    y, x = np.minimum(c["yt"] + dy, ih - 1), np.minimum(c["xl"] + dx, iw - 1)
    return np.where(inside[..., None], img64[b, y, x], 0.0)


def forward(img, grid_, mutate=None):
    """(value, S), float64, B x gh x gw x C (mutate: see cells)"""
    Bn, ih, iw, C = img.shape
    c = cells(grid_, ih, iw, mutate)
    img64 = img.astype(f64)
    val = np.zeros(grid_.shape[:3] + (C,), f64)
    S = np.zeros_like(val)
    for dy, dx, inside, wa, wb in _taps(c):
        term = (wa * wb)[..., None] * _gather(img64, c, dy, dx, inside)
        val += term
        S += np.abs(term)
    return val, S


def grid_gradient(img, grid_, grad_out, mutate=None):
    """(value, S), float64, B x gh x gw x 2 (x first): lines 287-288 on float64 dot products"""
    Bn, ih, iw, C = img.shape
    c = cells(grid_, ih, iw, mutate)
    img64, go = img.astype(f64), grad_out.astype(f64)
    dots, absdots = [], []
    for dy, dx, inside, _, _ in _taps(c):
        p = _gather(img64, c, dy, dx, inside) * go
        dots.append(p.sum(-1))
        absdots.append(np.abs(p).sum(-1))
    (tl, tr, bl, br), (Atl, Atr, Abl, Abr) = dots, absdots
    xw, yw, ux, uy = (c[k].astype(f64) for k in ("xw", "yw", "ux", "uy"))
    yf = -xw * tl + xw * bl - ux * tr + ux * br
    xf = -yw * tl + yw * tr - uy * bl + uy * br
    Sy = xw * Atl + xw * Abl + ux * Atr + ux * Abr          # the weights are >= 0
    Sx = yw * Atl + yw * Atr + uy * Abl + uy * Abr
    if mutate == "store-yx":          # the two components stored in the other order (:294-295)
        return np.stack([yf, xf], -1), np.stack([Sy, Sx], -1)
    return np.stack([xf, yf], -1), np.stack([Sx, Sy], -1)


def image_gradient(img_shape, grid_, grad_out, mutate=None):
    """(value, S, K), B x ih x iw x C: the float64 scatter, the sum of |terms| and the number of terms per element"""
    Bn, ih, iw, C = img_shape
    c = cells(grid_, ih, iw, mutate)
    go = grad_out.astype(f64)
    val = np.zeros(img_shape, f64)
    S = np.zeros(img_shape, f64)
    K = np.zeros(img_shape, np.int64)
    b = np.broadcast_to(np.arange(Bn)[:, None, None], c["xl"].shape)
    for dy, dx, inside, wa, wb in _taps(c):
        term = (wa * wb)[..., None] * go
        at = (b[inside], (c["yt"] + dy)[inside], (c["xl"] + dx)[inside])
        np.add.at(val, at, term[inside])
        np.add.at(S, at, np.abs(term[inside]))
        np.add.at(K, at, 1)
    return val, S, K


def measure(got, val, S):
    """glue_float64.measure: worst |got - val| / (2^-24 S); inf where got is not 0 on S = 0 or holds a NaN"""
    return GF.measure(got, val, S)


def distance(a, b, S):
    """worst |a - b| / (2^-24 S) between two float32 results, over S > 0"""
    pos = S > 0
    if not pos.any():
        return 0.0
    return float((np.abs(np.asarray(a, f64) - np.asarray(b, f64))[pos] / (U * S[pos])).max())


@functools.lru_cache(maxsize=None)
def reference(case, field):
    """everything a test needs of one case and field, computed once and shared (read-only): dict of img, grid, grad_out and the float64
    (value, S) pairs fwd, gg, and gi = (value, S, K)"""
    img, g, go = image(case), grid(field, case), grad_output(case)
    out = dict(img=img, grid=g, grad_out=go, fwd=forward(img, g), gg=grid_gradient(img, g, go), gi=image_gradient(img.shape, g, go))
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return out


def unit_inputs(case, field, k):
    """(I B x C x h x w, F B x 2 x h x w) for warpingUnit(I, k F) on a case whose grid has the image's size: F = the field / k in float32"""
    C, ih, iw, gh, gw = case
    assert (ih, iw) == (gh, gw)
    I = np.ascontiguousarray(np.transpose(image(case), (0, 3, 1, 2)))
    F = (np.transpose(grid(field, case), (0, 3, 1, 2)) / f32(k)).astype(f32)
    return I, np.ascontiguousarray(F)


# ---- what keeps a field from being vacuous -----------------------------------------------------------------------------------------------

def field_facts(case):
    """what `edges` and `far` reach together on one case: a dict of booleans"""
    C, ih, iw, gh, gw = case
    cs = [cells(grid(f, case), ih, iw) for f in ("edges", "far")]
    cat = lambda k: np.concatenate([c[k].reshape(-1) for c in cs])
    xc, yc, xl, yt, xw, yw = (cat(k) for k in ("xc", "yc", "xl", "yt", "xw", "yw"))
    return {
        "clamps left": bool((xc < 0).any()), "clamps right": bool((xc > iw - 1).any()),
        "clamps top": bool((yc < 0).any()), "clamps bottom": bool((yc > ih - 1).any()),
        "on column 0": bool((xc == 0).any()), "on the last column": bool((xc == iw - 1).any()),
        "on row 0": bool((yc == 0).any()), "on the last row": bool((yc == ih - 1).any()),
        "top-left tap on the last column": bool((xl == iw - 1).any()), "top-left tap on the last row": bool((yt == ih - 1).any()),
        "both weights 1": bool(((xw == 1) & (yw == 1)).any()),
        "a weight inside (0, 1) on x": bool(((xw > 0) & (xw < 1)).any()), "a weight inside (0, 1) on y": bool(((yw > 0) & (yw < 1)).any()),
        "an edge on x under a blend on y": bool(((xl == iw - 1) & (yw > 0) & (yw < 1)).any()),
        "an edge on y under a blend on x": bool(((yt == ih - 1) & (xw > 0) & (xw < 1)).any()),
    }
