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

Any graph shape (option dict `o` of weights.graph_opts, default the shipped one, for which every function gives what it gave before the
argument existed, bit for bit: tests/test_graph_displaced_cpu.py holds the digests).  The first table level and the number of levels come
from `o` (l_st = max(skip + 1, 1), pwc.lua:136).  The image warp of level l displaces by k2 * (the table's flow of level l) with
k2 = flownet_factor / 2^(l - l_st), or flownet_factor with rescale_flow (pwc.lua:440-444; graph_run's k2), and the table's flow is fs[l]
after `skip` bilinear upsamplings, each of which doubles the values with rescale_flow (pwc.lua:364-369,382-388): the flow bias of level l is
disp_px * DIRECTION / (k2 * that gain).  With residual = 1 the decoder's output is added to the upsampled flow of the level above
(pwc.lua:341-351), so the bias is the level's target minus what arrives from there.  With occ_input = 1 the occlusion decoder of level l
reads the upsampled map of level l + 1 (pwc.lua:300-304): the levels are calibrated coarsest first, with one oracle forward per level, each
on the weights the levels above have already been given.  The table's occlusion map is occs[l] after `skip` nearest upsamplings, so the
calibration reads every 2^skip-th value.

two_frame = 1 (pwc.lua:160-165,279-296), on the nine-channel input of this project (frames = 3): only the cost volume towards frame 3
exists, it alone feeds the flow decoder, and only frame 3's features are warped from level to level (f_i = ref, l_i = ref + 1).  The
occlusion decoder is still built (frames > 2), on that cost volume, the reference features and frame 3's features, and its softmax fills
the table's occlusion slots as in every other graph; both image warps are still built, iws[1] from minus the future flow (Hard) or from
the past flow (Soft), as without the option.  So every condition below is defined for a two_frame graph and all are applied.

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

The generic graphs: tests/test_graph_options_cpu.py's CASES (seed 5, disp_px 3, occ_spread 1; standard-normal input drawn from
default_rng(H + W + past_flow); sizes 2 x 4m x 6m and 1 x 3m x 5m, m = 2^(levels - 1)).  Per row: the occlusion scales a_l; the smallest and
largest share of a plane at or above the threshold over the levels whose plane holds >= 96 values; the largest share of a finest-level
plane within 1e-3 of it; the smallest and largest over levels and warps of max |k2 * flow| in pixels; the smallest share of samples
outside the map over the warps of the two coarsest levels; the largest |oracle - float64 witness| over the table.

  case                        kind  size       a_l (coarsest .. finest)          planes >= 0.6666   within 1e-3   warps: max px     outside     |oracle - f64|
  createModelMulti(nil)       hard  2x32x48   16 15                             28.6 .. 37.5 %     <= 1.56 %      4.68 ..  5.91    >= 10.2 %    3.9e-05
  createModelMulti(nil)       hard  1x24x40   19 16                             20.0 .. 40.0 %     <= 0.00 %      4.45 ..  5.16    >= 12.1 %    2.5e-05
  createModelMulti(nil)       soft  2x32x48   17 14                             25.0 .. 34.4 %     <= 0.00 %      3.42 ..  5.28    >= 10.2 %    3.2e-05
  createModelMulti(nil)       soft  1x24x40   24 17                             26.7 .. 33.3 %     <= 0.00 %      3.15 ..  4.83    >= 13.0 %    2e-05
  no_siamese                  hard  2x32x48   51 34                             26.0 .. 36.5 %     <= 0.00 %      3.13 ..  4.30    >= 15.3 %    1.7e-05
  no_siamese                  hard  1x24x40   50 31                             26.7 .. 40.0 %     <= 0.00 %      3.13 ..  4.32    >= 18.9 %    1.2e-05
  no_siamese                  soft  2x32x48   48 40                             26.6 .. 35.9 %     <= 0.00 %      3.15 ..  7.04    >= 16.9 %    1.8e-05
  no_siamese                  soft  1x24x40   42 42                             26.7 .. 40.0 %     <= 0.00 %      3.14 ..  6.75    >= 20.8 %    1.5e-05
  occ_input+rescale           hard  2x64x96   14 16 12                          27.1 .. 39.6 %     <= 0.39 %      4.74 .. 21.65    >=  7.6 %    0.0002
  occ_input+rescale           hard  1x48x80   18 19 13                          26.7 .. 40.0 %     <= 0.42 %      5.28 .. 19.39    >= 12.5 %    0.00014
  occ_input+rescale           soft  2x64x96   12 11 10                          30.7 .. 37.5 %     <= 0.52 %      4.77 .. 29.68    >= 11.3 %    0.00019
  occ_input+rescale           soft  1x48x80   17 14 11                          20.0 .. 40.0 %     <= 0.42 %      5.27 .. 28.30    >= 20.8 %    0.00012
  residual                    hard  2x64x96   16 12 11                          29.2 .. 35.4 %     <= 0.13 %      3.17 .. 16.50    >= 19.4 %    9e-05
  residual                    hard  1x48x80   35 11 12                          27.9 .. 34.6 %     <= 0.00 %      3.14 .. 14.47    >= 24.9 %    6.7e-05
  residual                    soft  2x64x96   15 11 8                           31.2 .. 35.4 %     <= 0.26 %      3.16 .. 16.11    >= 17.0 %    9.4e-05
  residual                    soft  1x48x80   30 11 8                           13.3 .. 46.7 %     <= 0.00 %      3.14 .. 13.61    >= 22.1 %    6.2e-05
  skip0                       hard  2x16x24   38 16 9                           30.7 .. 32.8 %     <= 0.52 %      3.17 .. 14.70    >= 49.5 %    5.9e-05
  skip0                       hard  1x12x20   42 15 9                           30.4 .. 32.9 %     <= 0.42 %      3.14 .. 13.34    >= 58.3 %    4e-05
  skip0                       soft  2x16x24   36 10 10                          30.2 .. 34.4 %     <= 0.39 %      3.11 .. 14.80    >= 50.5 %    4.3e-05
  skip0                       soft  1x12x20   47 12 11                          30.4 .. 35.4 %     <= 0.00 %      3.11 .. 13.34    >= 56.7 %    3.2e-05
  skip0+no_siamese+two_frame  hard  2x16x24   27 10 6                           30.7 .. 34.8 %     <= 0.26 %      3.47 .. 21.40    >= 41.7 %    0.00022
  skip0+no_siamese+two_frame  hard  1x12x20   39 12 6                           31.2 .. 31.7 %     <= 0.42 %      3.42 .. 23.17    >= 51.7 %    0.00019
  skip0+no_siamese+two_frame  soft  2x16x24   26 11 6                           30.2 .. 32.3 %     <= 0.39 %      3.35 .. 22.24    >= 31.8 %    0.00015
  skip0+no_siamese+two_frame  soft  1x12x20   24 14 6                           32.1 .. 34.6 %     <= 0.83 %      3.28 .. 20.06    >= 46.7 %    0.00015
  skip0+occ_input+rescale     hard  2x16x24   38 20 11                          30.2 .. 33.6 %     <= 0.52 %      3.70 ..  8.66    >= 26.0 %    4.8e-05
  skip0+occ_input+rescale     hard  1x12x20   42 17 11                          30.0 .. 33.3 %     <= 0.42 %      3.54 ..  7.61    >= 30.0 %    3.5e-05
  skip0+occ_input+rescale     soft  2x16x24   36 16 9                           31.2 .. 32.4 %     <= 0.52 %      3.42 ..  9.42    >= 49.0 %    5.5e-05
  skip0+occ_input+rescale     soft  1x12x20   47 17 9                           30.4 .. 32.5 %     <= 0.42 %      3.42 ..  9.72    >= 60.0 %    4.2e-05
  skip1+factor                hard  2x32x48   16 15 11                          30.2 .. 33.3 %     <= 0.26 %      3.08 ..  4.89    >= 14.3 %    2.7e-05
  skip1+factor                hard  1x24x40   41 17 12                          30.0 .. 32.5 %     <= 0.00 %      2.94 ..  4.84    >= 18.8 %    1.7e-05
  skip1+factor                soft  2x32x48   23 5 9                            29.2 .. 32.2 %     <= 0.26 %      3.03 ..  7.89    >= 27.7 %    2.5e-05
  skip1+factor                soft  1x24x40   28 6 13                           23.3 .. 36.7 %     <= 0.00 %      3.01 ..  7.37    >= 33.3 %    2.2e-05
  skip3                       hard  2x64x96   16 6                              28.1 .. 35.4 %     <= 0.52 %      2.81 .. 10.40    >=  8.5 %    7.5e-05
  skip3                       hard  1x48x80   35 6                              26.7 .. 36.7 %     <= 1.67 %      2.97 ..  6.51    >=  8.8 %    3e-05
  skip3                       soft  2x64x96   15 7                              29.2 .. 35.4 %     <= 0.52 %      2.81 ..  6.43    >=  2.8 %    4.9e-05
  skip3                       soft  1x48x80   30 9                              13.3 .. 46.7 %     <= 0.00 %      2.96 ..  5.81    >=  4.1 %    3.5e-05
  sum_cvs                     hard  2x64x96   14 11 11                          27.1 .. 39.6 %     <= 0.52 %      3.33 ..  6.63    >=  9.0 %    3.5e-05
  sum_cvs                     hard  1x48x80   18 15 13                          25.0 .. 40.0 %     <= 0.42 %      3.21 ..  5.96    >= 11.0 %    3.6e-05
  sum_cvs                     soft  2x64x96   12 12 13                          30.7 .. 37.5 %     <= 0.00 %      3.35 .. 11.40    >= 11.8 %    5.1e-05
  sum_cvs                     soft  1x48x80   17 11 13                          20.0 .. 40.0 %     <= 0.00 %      3.21 .. 10.36    >= 15.9 %    3.5e-05
  two_frame                   hard  2x32x48   35 14                             27.1 .. 35.4 %     <= 0.00 %      4.30 ..  7.10    >= 15.7 %    4e-05
  two_frame                   hard  1x24x40   24 17                             26.7 .. 33.3 %     <= 0.00 %      4.17 ..  6.80    >= 22.1 %    2.8e-05
  two_frame                   soft  2x32x48   20 10                             31.2 .. 32.3 %     <= 0.52 %      3.06 ..  8.83    >= 12.8 %    2.9e-05
  two_frame                   soft  1x24x40   46 9                              28.3 .. 33.3 %     <= 0.00 %      2.89 ..  7.11    >= 14.5 %    2.8e-05
one-pixel coarsest map (1 x m x m): |oracle - f64| <= 3.7e-05 (occ_input+rescale soft)

Every row meets every condition except (CASE_BOUNDS holds each of these cases to the bound in brackets, at both sizes and kinds):
  outside the map, two coarsest levels    sum_cvs 9.0 % [8.5 %], skip3 2.8 % [2.5 %]: these graphs have five levels, so their second
                                          coarsest level is level 4, whose table map is 32 x 48 (skip 2) or, for skip3 where level 4 is
                                          also the finest, 64 x 96 -- the shipped graph's is level 6 with 16 x 24 -- and 3 pixels of
                                          displacement take fewer than a tenth of such a map's samples over its edge; their coarsest
                                          level has 12 % or more outside in every row.  occ_input+rescale 7.6 % [7 %], at level 5 (16 x 24)
                                          of hard 2 x 64 x 96: with rescale_flow the decoders' network term is multiplied by 80 and
                                          outweighs the bias (up to 21 pixels), so the flow does not point one way across the map.
  within 1e-3 of the threshold            createModelMulti(nil) hard 2 x 32 x 48: 1.56 % [2 %]; skip3 hard 1 x 48 x 80: 1.67 % [2 %].  The
                                          finest table map is a nearest upsampling of 2 x 8 x 12 = 192 resp. 6 x 10 = 60 decoder values, so
                                          one value is 0.52 % resp. 1.67 % of the plane: three values resp. one value lie that close.
The rescale_flow and residual rows reach 10 .. 30 pixels: there the decoders' network term, which the bias does not set, is multiplied by
flownet_factor * 2^skip = 80 (rescale_flow) or summed over the levels (residual).
"""
import numpy as np

from back2future_amd import weights as W
from oracle import oracle as O

THR = 0.6666                 # occ_threshold of back2future.lua:40
L_ST, LEVELS = 3, 7          # of the shipped graph
DIRECTION = (1.0, -0.7)      # the bias points right and (less far) up, so that both clamps of both axes are met by flow / past


def oracle_opts(o, past_flow):
    """The oracle's option struct of an option dict (weights.graph_opts)"""
    return O.opts(past_flow, **{k: o[k] for k in ("win", "levels", "skip", "two_frame", "sum_cvs", "residual", "occ_input", "rescale_flow",
                                                   "flownet_factor", "siamese")})


def graph_levels(o=W.SHIPPED):
    """(first table level l_st, number of levels) of a graph (pwc.lua:136)"""
    return max(o["skip"] + 1, 1), o["levels"]


def warp_factor(l, o=W.SHIPPED):
    """k2 > 0 of level l: iws[3][l] samples its map at x + k2 * (the table's flow of level l), iws[1][l] at x - k2 * (...)
    (pwc.lua:440-444; graph_run's k2)"""
    return float(o["flownet_factor"]) if o["rescale_flow"] else float(o["flownet_factor"]) / 2.0 ** (l - graph_levels(o)[0])


def flow_gain(l, o=W.SHIPPED):
    """The table's flow of level l is fs[l] bilinearly upsampled max(skip, 0) times; rescale_flow doubles it at every upsampling
    (pwc.lua:364-369,382-388): its values are those of fs[l] times this."""
    return 2.0 ** o["skip"] if o["rescale_flow"] else 1.0


def set_flow_bias(flat, past_flow, bias, o=W.SHIPPED):
    """conv6.b of every flow decoder = bias, of every past-flow decoder = -bias (in place; returns flat).  bias: one (u, v) pair for
    all levels, or a function of the level."""
    for name, shape, off in W.layout(past_flow, o)[0]:
        if name.endswith(".conv6.b") and (".flow." in name or ".past." in name):
            b = bias(int(name[1:name.index(".")])) if callable(bias) else bias
            flat[off:off + 2] = np.asarray(b, np.float32) * (1.0 if ".flow." in name else -1.0)
    return flat


def level_bias(disp_px, o=W.SHIPPED):
    """The bias under which fs[l] is about disp_px * DIRECTION pixels of the map that the image warp of level l samples: disp_px / (k2 *
    flow_gain).  With residual = 1 the decoder's output is added to the upsampled flow of the level above (pwc.lua:341-351), so its bias is
    the level's target minus what arrives from above (the target of level l + 1, doubled by rescale_flow's upsampling)."""
    l_st, levels = graph_levels(o)
    ff = float(o["flownet_factor"])

    def target(l, d):
        if o["rescale_flow"]:
            return disp_px * d * 2.0 ** -o["skip"] / ff
        return disp_px * d * 2.0 ** (l - l_st) / ff

    def bias(l):
        if o["residual"] and l < levels:
            up = 2.0 if o["rescale_flow"] else 1.0
            return tuple(target(l, d) - up * target(l + 1, d) for d in DIRECTION)
        return tuple(target(l, d) for d in DIRECTION)
    return bias


def table_index(past_flow, l, what, o=W.SHIPPED):
    """Position in model:forward's table (pwc.lua:459-489) of 'ufs', 'ubfs' (Soft), 'occs', 'iw1', 'iw3' of level l."""
    names = ["ufs", "ubfs", "occs", "iw1", "iw3"] if past_flow else ["ufs", "occs", "iw1", "iw3"]
    return (l - graph_levels(o)[0]) * len(names) + names.index(what)


def logit_difference(occ):
    """log(p1 / p0) of a B x 2 x h x w probability map, in float64"""
    p = occ.astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p[:, 1]) - np.log(p[:, 0])


def displaced_weights(seed, past_flow, x, disp_px=3.0, occ_spread=1.0, gain=2.0, report=None, o=W.SHIPPED):
    """Canonical flat weights (see the module docstring).  x: B x 9 x H x W normalized input the occlusion heads are calibrated on.
    report (a dict) receives {level: (a_l, b1)}."""
    l_st, levels = graph_levels(o)
    oo = oracle_opts(o, past_flow)
    flat = W.random_init(seed, past_flow, gain, o)
    set_flow_bias(flat, past_flow, level_bias(disp_px, o), o)
    v = W.views(flat, past_flow, o)
    step = 1 << o["skip"]                    # the table's map is occs[l] after skip nearest upsamplings (pwc.lua:311-321,468-470)
    table = O.pwc_forward(x, flat, past_flow, oo)
    for l in range(levels, l_st - 1, -1):
        if o["occ_input"] and l < levels:    # this level reads the map of the level above, which has just changed
            table = O.pwc_forward(x, flat, past_flow, oo)
        w, b = v["l%d.occ.conv6.w" % l], v["l%d.occ.conv6.b" % l]
        n = logit_difference(table[table_index(past_flow, l, "occs", o)])[:, ::step, ::step] - (float(b[1]) - float(b[0]))
        q1, med, q3 = np.percentile(n, [25, 50, 75])
        a = occ_spread / (0.5 * (q3 - q1))
        w *= np.float32(a)
        b[1] = np.float32(-0.5 * a * med)
        b[0] = -b[1]
        if report is not None:
            report[l] = (float(a), float(b[1]))
    return flat


def conditions(table, past_flow, o=W.SHIPPED, bounds=None):
    """What the oracle's table must show for a test on these weights to mean anything; returns (list of failures, list of report lines).

    - occlusion: in each plane of the table's occlusion map of level l, at every level whose map holds at least 96 values per plane,
      between 10 % and 60 % of the values are at or above 0.6666 (the planes exclude each other); on smaller maps each plane holds a value
      on each side;
    - at most 1 % of the values of a plane of the finest level lie within 1e-3 of 0.6666 (the ones a mask comparison may skip);
    - |k2 * flow| (and the past flow for Soft) exceeds 2 pixels somewhere at every level, and at the two coarsest levels at least a
      tenth of the image-warp samples of each frame fall outside the map (through the clamp).

    bounds: a case that cannot meet a condition states its own bound, taken from the measurement in the module docstring's table:
    {"share": (lo, hi), "near": x, "far": px, "outside": share}; a key that is absent keeps the bound above."""
    bounds = dict({"share": (0.10, 0.60), "near": 0.01, "far": 2.0, "outside": 0.10}, **(bounds or {}))
    l_st, levels = graph_levels(o)
    bad, lines = [], []
    for l in range(l_st, levels + 1):
        occ = table[table_index(past_flow, l, "occs", o)]
        k2 = warp_factor(l, o)
        for c in (0, 1):
            plane = occ[:, c]
            share = float((plane >= THR).mean())
            near = float((np.abs(plane - THR) < 1e-3).mean())
            lines.append("level %d occ plane %d: %5.1f %% >= thr, %5.2f %% within 1e-3, range %.4g .. %.4g" % (l, c, 100 * share, 100 * near, plane.min(), plane.max()))
            if plane[0].size >= 96:
                if not bounds["share"][0] <= share <= bounds["share"][1]:
                    bad.append("level %d plane %d: %.3f of the values >= thr" % (l, c, share))
            elif not ((plane >= THR).any() and (plane < THR).any()):
                bad.append("level %d plane %d: one-sided" % (l, c))
            if l == l_st and near > bounds["near"]:
                bad.append("level %d plane %d: %.4f of the values within 1e-3 of thr" % (l, c, near))
        for what, sign in [("ufs", 1.0)] + ([("ubfs", -1.0)] if past_flow else [("ufs", -1.0)]):
            f = table[table_index(past_flow, l, what, o)].astype(np.float64) * (k2 * sign)     # the displacement of iw3 (sign +) / iw1 (-)
            h, w = f.shape[-2:]
            xs, ys = np.arange(w)[None, None, :] + f[:, 0], np.arange(h)[None, :, None] + f[:, 1]
            out = float(((xs < 0) | (xs > w - 1) | (ys < 0) | (ys > h - 1)).mean())
            far = float(np.abs(f).max())
            lines.append("level %d %s x %+.3g: |displacement| <= %.2f px of the %d x %d map, %4.1f %% of the samples outside" % (l, what, k2 * sign, far, h, w, 100 * out))
            if far <= bounds["far"]:
                bad.append("level %d %s: displacement %.3f px <= %g" % (l, what, far, bounds["far"]))
            if l >= levels - 1 and out < bounds["outside"]:
                bad.append("level %d %s: %.3f of the samples outside the map" % (l, what, out))
    return bad, lines


def assert_conditions(table, past_flow, o=W.SHIPPED, bounds=None):
    bad, lines = conditions(table, past_flow, o, bounds)
    assert not bad, "\n".join(bad + lines)
    return lines


# Cases of tests/test_graph_options_cpu.py's CASES that cannot meet a condition above, with the bound each is held to instead; the
# measured figures and the reasons are in the module docstring's table of the generic graphs.
CASE_BOUNDS = {
    "createModelMulti(nil)": {"near": 0.02},
    "occ_input+rescale": {"outside": 0.07},
    "sum_cvs": {"outside": 0.085},
    "skip3": {"near": 0.02, "outside": 0.025},
}
