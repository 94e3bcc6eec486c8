"""Weights under which every level moves its warps by whole pixels and the occlusion softmax decides.

`random:{hard,soft}:<seed>:2.0` leaves two families of kernels near their trivial point: the image warps of levels 5..7 stay inside one
pixel, and the occlusion probabilities stay inside 0.3 .. 0.7, so the masks are constant or nearly so.  Today's numbers for
`random:soft:5:2.0` (oracle, 128 x 192): on the smooth [0, 1] triplet of tests/test_gpu_displaced.py est3 lies in 0.416 .. 0.584 and both
masks are empty (0 of 24 576 pixels set); the image warps move by at most 5.1 / 1.8 / 0.71 / 0.19 / 0.06 pixels of their map at levels
3..7.  On standard-normal input: est3 in 0.337 .. 0.663, 6.7 / 3.2 / 0.85 / 0.20 / 0.06 pixels (Hard: 6.1 / 3.9 / 1.9 / 0.55 / 0.06).

`displaced_weights` starts from `weights.random_init` and changes the last layer of the decoders only:

  flow / past   conv6.b of level l = +/- disp_px * (1, -0.7) * 2^(l-3) / 20: the image warp of level l multiplies skip_ufs[l] by
                k2 = 20 / 2^(l-3) (pwc.lua:443), so every level predicts about disp_px pixels of the map its image warp samples (half
                of that on the feature map the next level warps).  One bias for all levels cannot do this: (0.35, -0.25) gives
                11.7 / 5.8 / 2.1 / 0.95 / 0.52 pixels at levels 3..7.
  occ           conv6.w scaled by a_l and conv6.b replaced so that the logit difference d = z1 - z0 = log(p1 / p0) of level l has
                median 0 and quartiles about +/- occ_spread on the input x.  d = a * n + (b1 - b0) with n the network term, which the
                CPU oracle gives as log(p1 / p0) of skip_occs[l] minus the bias difference it ran with: a_l = occ_spread / (half the
                inter-quartile range of n), b1 = -b0 = -a_l * median(n) / 2.  In the shipped graph (pwc_occ_input = 0) no layer reads an
                occlusion map, so the levels do not depend on each other and one oracle forward serves all five; everything is
                computed on the CPU from the oracle, never from GPU output.

`conditions` states what the tests need of the oracle's own output before they compare anything (see its docstring); every test calls
`assert_conditions` first.

Measured with the oracle (seed 5, disp_px 3, occ_spread 1; input of tests/test_gpu_displaced.py's table tests: standard normal,
default_rng(H + W + past_flow)).  a_l, b1: what the calibration set (b0 = -b1); share of each plane at or above the threshold; share
within 1e-3 of it; largest |k2 * flow| in pixels of the map and share of samples outside it, for the warp of frame 3 (k2 > 0) and of
frame 1 (k2 < 0; skip_ubfs for Soft).  The [0, 1] inputs of the three-output tests give the same picture (31 .. 34 % of each level-3
plane over the threshold for Soft, final flow 3.5 (Hard) / 6.3 (Soft) pixels).

hard 2 x 128 x 192
  level  scale a_l   bias b1   plane 0 / 1 >= 0.6666   within 1e-3   fwd warp: max px, outside   frame-1 warp: max px, outside
  3          16.2    -1.850    31.9 % / 31.0 %          0.16 / 0.26 %        4.50    4.0 %               4.50    1.2 %
  4          20.5    -0.200    32.9 % / 31.2 %          0.00 / 0.13 %        4.82    7.4 %               4.82    8.9 %
  5          19.6    +0.880    32.3 % / 32.8 %          0.52 / 0.00 %        3.61   12.9 %               3.61   12.4 %
  6          62.6    -1.073    27.1 % / 35.4 %          0.00 / 0.00 %        3.30   28.9 %               3.30   32.3 %
  7         160.4    +6.790    33.3 % / 25.0 %          0.00 / 0.00 %        3.08   58.3 %               3.08   58.3 %
hard 1 x 192 x 320
  level  scale a_l   bias b1   plane 0 / 1 >= 0.6666   within 1e-3   fwd warp: max px, outside   frame-1 warp: max px, outside
  3          17.2    -1.994    32.2 % / 31.9 %          0.10 / 0.13 %        4.12    2.5 %               4.12    0.8 %
  4          19.1    -0.135    31.0 % / 31.7 %          0.31 / 0.21 %        4.43    4.9 %               4.43    5.9 %
  5          26.1    +1.215    29.2 % / 35.4 %          0.42 / 0.00 %        3.57    8.5 %               3.57    7.8 %
  6          58.1    -1.461    31.7 % / 36.7 %          0.00 / 0.00 %        3.31   19.1 %               3.31   20.9 %
  7          61.6    +3.458    40.0 % / 33.3 %          0.00 / 0.00 %        3.11   40.0 %               3.11   40.0 %
soft 2 x 128 x 192
  level  scale a_l   bias b1   plane 0 / 1 >= 0.6666   within 1e-3   fwd warp: max px, outside   frame-1 warp: max px, outside
  3          13.7    +2.630    31.1 % / 32.3 %          0.16 / 0.23 %        7.34    3.4 %               8.30    2.2 %
  4          12.5    +1.713    33.5 % / 32.8 %          0.13 / 0.26 %        5.50    8.6 %               5.76   10.8 %
  5          23.4    +1.311    28.1 % / 32.8 %          0.00 / 0.52 %        3.43   16.1 %               3.86   16.6 %
  6          34.4    +0.794    35.4 % / 22.9 %          0.00 / 0.00 %        3.17   28.9 %               3.34   27.2 %
  7         137.2    +5.586    33.3 % / 16.7 %          0.00 / 0.00 %        3.08   58.3 %               3.03   56.2 %
soft 1 x 192 x 320
  level  scale a_l   bias b1   plane 0 / 1 >= 0.6666   within 1e-3   fwd warp: max px, outside   frame-1 warp: max px, outside
  3          14.3    +2.799    31.0 % / 32.6 %          0.13 / 0.44 %        7.65    2.1 %               8.40    1.3 %
  4          14.2    +2.105    30.6 % / 32.7 %          0.21 / 0.00 %        5.44    5.4 %               5.69    7.1 %
  5          22.2    +1.492    28.3 % / 35.4 %          0.00 / 0.42 %        3.45   10.2 %               3.81   10.5 %
  6          21.3    +0.967    35.0 % / 35.0 %          0.00 / 0.00 %        3.21   19.1 %               3.50   17.6 %
  7          42.9    +2.369    46.7 % / 26.7 %          0.00 / 0.00 %        3.11   40.0 %               3.03   36.2 %
"""
import numpy as np

from back2future_amd import weights as W
from oracle import oracle as O

THR = 0.6666                 # occ_threshold of back2future.lua:40
L_ST, LEVELS = 3, 7
DIRECTION = (1.0, -0.7)      # the bias points right and (less far) up, so that both clamps of both axes are met by flow / past


def set_flow_bias(flat, past_flow, bias, o=W.SHIPPED):
    """conv6.b of every flow decoder = bias, of every past-flow decoder = -bias (in place; returns flat).  bias: one (u, v) pair for
    all levels, or a function of the level."""
    for name, shape, off in W.layout(past_flow, o)[0]:
        if name.endswith(".conv6.b") and (".flow." in name or ".past." in name):
            b = bias(int(name[1:name.index(".")])) if callable(bias) else bias
            flat[off:off + 2] = np.asarray(b, np.float32) * (1.0 if ".flow." in name else -1.0)
    return flat


def level_bias(disp_px):
    return lambda l: (disp_px * DIRECTION[0] * 2.0 ** (l - L_ST) / 20.0, disp_px * DIRECTION[1] * 2.0 ** (l - L_ST) / 20.0)


def table_index(past_flow, l, what):
    """Position in model:forward's table (pwc.lua:459-489) of 'ufs', 'ubfs' (Soft), 'occs', 'iw1', 'iw3' of level l."""
    names = ["ufs", "ubfs", "occs", "iw1", "iw3"] if past_flow else ["ufs", "occs", "iw1", "iw3"]
    return (l - L_ST) * len(names) + names.index(what)


def logit_difference(occ):
    """log(p1 / p0) of a B x 2 x h x w probability map, in float64"""
    p = occ.astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p[:, 1]) - np.log(p[:, 0])


def displaced_weights(seed, past_flow, x, disp_px=3.0, occ_spread=1.0, gain=2.0, report=None):
    """Canonical flat weights (see the module docstring).  x: B x 9 x H x W normalized input the occlusion heads are calibrated on.
    report (a dict) receives {level: (a_l, b1)}."""
    flat = W.random_init(seed, past_flow, gain)
    set_flow_bias(flat, past_flow, level_bias(disp_px))
    v = W.views(flat, past_flow)
    table = O.pwc_forward(x, flat, past_flow)
    for l in range(LEVELS, L_ST - 1, -1):
        w, b = v["l%d.occ.conv6.w" % l], v["l%d.occ.conv6.b" % l]
        n = logit_difference(table[table_index(past_flow, l, "occs")])[:, ::4, ::4] - (float(b[1]) - float(b[0]))
        q1, med, q3 = np.percentile(n, [25, 50, 75])
        a = occ_spread / (0.5 * (q3 - q1))
        w *= np.float32(a)
        b[1] = np.float32(-0.5 * a * med)
        b[0] = -b[1]
        if report is not None:
            report[l] = (float(a), float(b[1]))
    return flat


def conditions(table, past_flow):
    """What the oracle's table must show for a test on these weights to mean anything; returns (list of failures, list of report lines).

    - occlusion: in each plane of skip_occs[l], at every level whose map holds at least 96 values per plane, between 10 % and 60 % of the
      values are at or above 0.6666 (the planes exclude each other); on smaller maps each plane holds a value on each side;
    - at most 1 % of the level-3 values of a plane lie within 1e-3 of 0.6666 (the ones a mask comparison may skip);
    - |k2 * skip_ufs[l]| (and skip_ubfs for Soft) exceeds 2 pixels somewhere at every level, and at the two coarsest levels at least a
      tenth of the image-warp samples of each frame fall outside the map (through the clamp)."""
    bad, lines = [], []
    for l in range(L_ST, LEVELS + 1):
        occ = table[table_index(past_flow, l, "occs")]
        k2 = 20.0 / 2.0 ** (l - L_ST)
        for c in (0, 1):
            plane = occ[:, c]
            share = float((plane >= THR).mean())
            near = float((np.abs(plane - THR) < 1e-3).mean())
            lines.append("level %d occ plane %d: %5.1f %% >= thr, %5.2f %% within 1e-3, range %.4g .. %.4g" % (l, c, 100 * share, 100 * near, plane.min(), plane.max()))
            if plane[0].size >= 96:
                if not 0.10 <= share <= 0.60:
                    bad.append("level %d plane %d: %.3f of the values >= thr" % (l, c, share))
            elif not ((plane >= THR).any() and (plane < THR).any()):
                bad.append("level %d plane %d: one-sided" % (l, c))
            if l == L_ST and near > 0.01:
                bad.append("level 3 plane %d: %.4f of the values within 1e-3 of thr" % (c, near))
        for what, sign in [("ufs", 1.0)] + ([("ubfs", -1.0)] if past_flow else [("ufs", -1.0)]):
            f = table[table_index(past_flow, l, what)].astype(np.float64) * (k2 * sign)     # the displacement of iw3 (sign +) / iw1 (-)
            h, w = f.shape[-2:]
            xs, ys = np.arange(w)[None, None, :] + f[:, 0], np.arange(h)[None, :, None] + f[:, 1]
            out = float(((xs < 0) | (xs > w - 1) | (ys < 0) | (ys > h - 1)).mean())
            far = float(np.abs(f).max())
            lines.append("level %d %s x %+.3g: |displacement| <= %.2f px of the %d x %d map, %4.1f %% of the samples outside" % (l, what, k2 * sign, far, h, w, 100 * out))
            if far <= 2.0:
                bad.append("level %d %s: displacement %.3f px <= 2" % (l, what, far))
            if l >= LEVELS - 1 and out < 0.10:
                bad.append("level %d %s: %.3f of the samples outside the map" % (l, what, out))
    return bad, lines


def assert_conditions(table, past_flow):
    bad, lines = conditions(table, past_flow)
    assert not bad, "\n".join(bad + lines)
    return lines
