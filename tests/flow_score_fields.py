"""Shared by tests/test_flow_score_cpu.py and tests/test_gpu_flow_score.py: the fields the flow scores are tested on and the plain
numpy restatement of include/b2f.h's definition (fp64, one expression per counter) that the host entry is held against."""
import numpy as np

WORDS = 22
PIXELS, EPE_Q20, OUTLIERS, OCC, NONFINITE = 0, 4, 8, 12, 21
SCALE = 20.0


def _next(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def _prev(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


# (fx, fy, gx, gy, valid, gt_occ, p0, p1): the pixels every field of at least 64 pixels carries in each image, flow_scale = 20.
# 0.05 * 100.0 is 5.0 exactly in fp64, and 102.5 - 99.5, 12.5 - 9.5 and 105 - 100 are exact.
SPECIAL = [
    (5.125, 0.0, 99.5, 0.0, 1, 1, 0.75, 0.25),            # err == 3.0, 0.05 |gt| = 4.975 above it: no outlier; (1 - p0) + p1 == 0.5 -> class 1
    (0.625, 0.0, 9.5, 0.0, 1, 1, 0.25, 0.75),             # err == 3.0, 0.05 |gt| = 0.475 below it: no outlier (err > 3 fails); 1.5 -> class 2
    (0.625, 0.0, _prev(9.5), 0.0, 1, 0, 0.75, 0.25),      # err just above 3, 0.05 |gt| below: outlier
    (5.125, 0.0, _prev(99.5), 0.0, 1, 2, 0.25, 0.75),     # err just above 3, 0.05 |gt| above: no outlier
    (5.25, 0.0, 100.0, 0.0, 1, 1, -3.0, 2.0),             # err == 5.0 == 0.05 |gt|: no outlier; 6 clamps to class 2
    (_next(5.25), 0.0, 100.0, 0.0, 1, 1, 5.0, 0.0),       # err just above 0.05 |gt|, above 3: outlier; -4 clamps to class 0
    (0.0, 1e4, 0.0, 0.0, 1, 2, 0.5, 0.5),                 # err = 2e5 px: saturates at 65536
    (3.3e37, 0.0, 0.0, 0.0, 1, 3, 0.5, 0.5),              # err = 6.6e38, beyond fp32 but finite in fp64: saturates; label 3
    (0.1, 0.2, 1e9, 1e9, 0, 1, 0.9, 0.05),                # Sintel's unknown marker under valid == 0: no effect on the flow words
    (0.1, 0.2, np.nan, 1.0, 0, 0, 0.05, 0.9),             # NaN ground truth under valid == 0: no effect
    (np.nan, 0.2, 1.0, 1.0, 0, 255, 0.5, 0.5),            # NaN flow under valid == 0, unlabelled
    (0.1, 0.2, np.nan, 1.0, 1, 1, 0.2, 0.1),              # NaN under valid != 0: nonfinite only
    (np.nan, np.nan, 1.0, 1.0, 7, 3, 0.2, 0.1),           # the same with another nonzero mask byte, label 3
    (np.inf, 0.0, np.inf, 0.0, 255, 2, 0.2, 0.1),         # inf - inf = NaN: nonfinite
    (0.05, 0.05, 1.0, 1.0, 1, 255, 0.9, 0.9),             # label 255: bucket 3, not in the matrix
    (0.05, 0.05, 1.0, 1.0, 1, 3, 0.9, 0.9),               # label 3
]


def fields(H, W, n=3, seed=0):
    """flow, gt_flow, occ_prob (float32 n x 2 x H x W), valid, gt_occ (uint8 n x H x W): random fields whose errors straddle the Fl
    rule, with the SPECIAL pixels in every image (images under 64 pixels hold special pixels only, other ones from image to image)."""
    r = np.random.default_rng(seed * 7919 + H * 1000 + W)
    hw = H * W
    flow = r.normal(0, 0.3, (n, 2, hw)).astype(np.float32)
    gt = (flow * np.float32(SCALE) + r.normal(0, 2.5, (n, 2, hw)) * r.choice([0.2, 1.0, 4.0], (n, 1, hw))).astype(np.float32)
    prob = r.random((n, 2, hw), dtype=np.float32)
    valid = r.choice(np.array([0, 1, 1, 1, 255, 2], np.uint8), (n, hw))
    occ = r.choice(np.array([0, 1, 1, 1, 2, 2, 3, 255, 77], np.uint8), (n, hw))
    def put(b, i, px):
        flow[b, :, i] = px[0:2]
        gt[b, :, i] = px[2:4]
        valid[b, i], occ[b, i] = px[4], px[5]
        prob[b, :, i] = px[6:8]
    for b in range(n):
        if hw >= 64:   # every special pixel, at places that differ from image to image (j * 37 is distinct modulo hw for j < 16)
            for j, px in enumerate(SPECIAL):
                put(b, (j * 37 + 5 * b + 3) % hw, px)
        else:          # a tiny image: its pixels are special ones, other ones in every image
            for i in range(hw):
                put(b, i, SPECIAL[(i + 5 * b + 1) % len(SPECIAL)])
    shape4, shape3 = (n, 2, H, W), (n, H, W)
    return flow.reshape(shape4), gt.reshape(shape4), prob.reshape(shape4), valid.reshape(shape3), occ.reshape(shape3)


def _round_half_away(s):
    """roundf on a float32 array without going through a wider type: trunc, then the exactly computed fraction decides"""
    t = np.trunc(s)
    return t + np.where(np.abs(s - t) >= np.float32(0.5), np.sign(s), np.float32(0)).astype(np.float32)


def numpy_scores(flow, gt_flow, occ_prob=None, valid=None, gt_occ=None, flow_scale=SCALE):
    """include/b2f.h's definition restated with numpy: fp64, one expression per counter."""
    n, _, H, W = flow.shape
    out = np.zeros((n, WORDS), np.uint64)
    for b in range(n):
        fx, fy = flow[b, 0].astype(np.float64), flow[b, 1].astype(np.float64)
        gx, gy = gt_flow[b, 0].astype(np.float64), gt_flow[b, 1].astype(np.float64)
        v = np.ones((H, W), bool) if valid is None else valid[b] != 0
        k = np.full((H, W), 3) if gt_occ is None else np.minimum(gt_occ[b].astype(np.int64), 3)
        with np.errstate(all="ignore"):
            dx, dy = fx * flow_scale - gx, fy * flow_scale - gy
            err = np.sqrt(dy * dy + dx * dx)
            mag = np.sqrt(gy * gy + gx * gx)
            nan = np.isnan(err)
            counted = v & ~nan
            q20 = np.where(counted, np.minimum(np.where(nan, 0.0, err), 65536.0) * 1048576.0 + 0.5, 0.0).astype(np.uint64)
            outlier = counted & (err > 3.0) & (err > 0.05 * mag)
        for j in range(4):
            out[b, PIXELS + j] = np.count_nonzero(counted & (k == j))
            out[b, EPE_Q20 + j] = q20[counted & (k == j)].sum(dtype=np.uint64)
            out[b, OUTLIERS + j] = np.count_nonzero(outlier & (k == j))
        out[b, NONFINITE] = np.count_nonzero(v & nan)
        if gt_occ is not None and occ_prob is not None:
            with np.errstate(all="ignore"):
                c = _round_half_away((np.float32(1.0) - occ_prob[b, 0]) + occ_prob[b, 1])
            cls = np.where(c >= 2, 2, np.where(c >= 1, 1, 0))
            for g in range(3):
                for e in range(3):
                    out[b, OCC + 3 * g + e] = np.count_nonzero((gt_occ[b] == g) & (cls == e))
    return out


def combos():
    """(use valid, use gt_occ, use occ_prob): with and without each of the optional planes"""
    return [(v, o, p) for v in (True, False) for o in (True, False) for p in (True, False)]


def pick(fl, use_valid, use_occ, use_prob):
    """keyword arguments of ops.flow_score / numpy_scores for a combination"""
    flow, gt, prob, valid, occ = fl
    return dict(occ_prob=prob if use_prob else None, valid=valid if use_valid else None, gt_occ=occ if use_occ else None)
