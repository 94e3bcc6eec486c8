"""GPU: the forward under multi-pixel flows at every level and occlusion logits that decide (tests/displaced.py).

Every expected value is the CPU oracle's on the same weights and input, a float64 restatement of one operation on the GPU's own
operands, or the 1e-3 contract of BASELINE.json; nothing is measured against another entry of the library unless that entry is itself
held against the oracle in the same test.  Each test first asserts displaced.conditions on the oracle's output: whole-pixel warps through
the clamp at every level, both mask values in every occlusion plane.  Run with -s to see the per-tensor figures (profiles/r08_displaced.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest

from back2future_amd import _lib, back2future, weights as W
from oracle import oracle as O
from tests import displaced as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_float_outputs import _nearest  # noqa: E402  (the index rule of image.scale 'simple' in numpy)
from tests.test_gpu_sequence import _outs, _run_sequence, _run_triplets, _triplets  # noqa: E402

SEED, DISP, SPREAD = 5, 3.0, 1.0
BAR = 1e-3                      # BASELINE.json: max-abs on flow / occlusion probabilities / the output table
THR = D.THR
EPS = 2.0 ** -23                # ulp of 1.0f
KINDS = ["hard", "soft"]
TABLE_SIZES = [(2, 128, 192), (1, 192, 320)]     # 192 x 320: the level-7 map is 3 x 5


def _model(which, flat):
    m = back2future.Model("random:%s:%d:2.0" % (which, SEED))
    m.set_weights(flat)
    return m


def _names(past):
    per = ["skip_ufs", "skip_ubfs", "skip_occs", "iws1", "iws3"] if past else ["skip_ufs", "skip_occs", "iws1", "iws3"]
    return ["%s[%d]" % (n, l) for l in range(3, 8) for n in per]


@functools.lru_cache(maxsize=None)
def _table_case(which, B, H, Wd, spread=SPREAD):
    """(x, weights, the oracle's table, the GPU's table) of one size; computed once per session"""
    past = which == "soft"
    x = np.random.default_rng(H + Wd + past).standard_normal((B, 9, H, Wd)).astype(np.float32)
    flat = D.displaced_weights(SEED, past, x, DISP, spread)
    exp = O.pwc_forward(x, flat, past)
    m = _model(which, flat)
    try:
        got = m.forward(x)
    finally:
        m.close()
    assert len(got) == len(exp) == (25 if past else 20)
    return x, flat, exp, got


# ---- (a) the whole table against the oracle ----

@pytest.mark.parametrize("B,H,Wd", TABLE_SIZES)
@pytest.mark.parametrize("which", KINDS)
def test_full_table_vs_oracle(which, B, H, Wd):
    past = which == "soft"
    x, flat, exp, got = _table_case(which, B, H, Wd)
    for line in D.assert_conditions(exp, past):
        print("conditions %s %dx%dx%d: %s" % (which, B, H, Wd, line))
    worst = []
    for name, a, b in zip(_names(past), got, exp):
        assert a.shape == b.shape and np.isfinite(a).all(), name
        err = float(np.abs(a.astype(np.float64) - b).max())
        print("table %s %dx%dx%d %-13s max|gpu - oracle| = %.3g  (max|oracle| = %.3g)" % (which, B, H, Wd, name, err, float(np.abs(b).max())))
        if not err <= BAR:
            worst.append((name, err))
    assert not worst, worst


# ---- (a') the whole table under every kernel a user can select ----

# Each setting also gets adaptive_kernels = 0 unless it sets that option.  Second entry: the profile tag (kKernels, csrc/b2f_api.hip) that
# the first layer of the level-3 decoders -- two K segments, the record behind a permuted cin_map -- must run under, or None.
KERNEL_SETTINGS = {
    "f4x4": ({"wino4_min_pixels": 0, "wino6": 0}, "W4"),
    "f6x6": ({"wino4_min_pixels": 0, "wino6": 1, "wino6_min_pixels": 0}, "W6"),
    "wino1d-1": ({"wino4_min_pixels": 0, "wino6": 0, "wino1d": 1}, "V1"),
    "wino1d-2": ({"wino4_min_pixels": 0, "wino6": 0, "wino1d": 2}, "V1"),
    "bf16-wide": ({"wino4_min_pixels": 0, "bf16_conv": 3, "bf16_conv_min_pixels": 0}, "E1"),
    "bf16_conv-0": ({"bf16_conv": 0}, None),
    "s2_loader-0": ({"s2_loader": 0}, None),
    "s2_loader-2": ({"s2_loader": 2}, None),
    "adaptive": ({"adaptive_kernels": 1}, None),
    "corr-0": ({"corr_variant": 0}, None),
    "corr-1": ({"corr_variant": 1}, None),
    "corr-3": ({"corr_variant": 3}, None),
    "corr-5": ({"corr_variant": 5}, None),
    "corr-7": ({"corr_variant": 7}, None),
}
# stride-2 layers of the pyramid (32 -> 64 ... 128 -> 192): the tags that must and must not appear
STRIDE2_TAGS = {"bf16_conv-0": (["D2"], ["E2", "L2"]), "s2_loader-0": (["E2"], ["L2", "D2"]), "s2_loader-2": (["L2"], ["E2", "D2"])}

_table_models = {}


def _table_model(which, B, H, Wd):
    """one context per model kind for the settings below, reloaded when the size (and with it the calibrated weights) changes"""
    m, key = _table_models.get(which, (None, None))
    if m is None:
        m = back2future.Model("random:%s:%d:2.0" % (which, SEED))
    if key != (B, H, Wd):
        m.set_weights(_table_case(which, B, H, Wd)[1])
        _table_models[which] = (m, (B, H, Wd))
    return m


@pytest.fixture(scope="module", autouse=True)
def _close_table_models():
    yield
    for m, _ in _table_models.values():
        m.close()
    _table_models.clear()


@pytest.mark.parametrize("setting", list(KERNEL_SETTINGS))
@pytest.mark.parametrize("B,H,Wd", TABLE_SIZES)
@pytest.mark.parametrize("which", KINDS)
def test_full_table_vs_oracle_under_every_kernel(which, B, H, Wd, setting):
    """The contract of test_full_table_vs_oracle with the stride-1 layers, the stride-2 layers and the cost volume on each kernel an option
    can put them on.  The full table is the only place where the past-flow decoders and flow_b run; at these sizes every map is below
    wino4_min_pixels, so without the options all of it runs on the small-map kernels.  The profile rows say which kernel ran."""
    past = which == "soft"
    x, flat, exp, _ = _table_case(which, B, H, Wd)
    D.assert_conditions(exp, past)
    opts, tag = KERNEL_SETTINGS[setting]
    m = _table_model(which, B, H, Wd)
    with m.options(**dict({"adaptive_kernels": 0}, **opts)), m.options(profile=1, profile_layers=1):
        m.profile_reset()
        got = m.forward(x)
        rows = {n: cnt for n, (ms, cnt) in m.profile_read().items() if cnt > 0}
    assert len(got) == len(exp)
    worst = []
    for name, a, b in zip(_names(past), got, exp):
        assert a.shape == b.shape and np.isfinite(a).all(), name
        err = float(np.abs(a.astype(np.float64) - b).max())
        print("table %s %dx%dx%d %-12s %-13s max|gpu - oracle| = %.3g  (max|oracle| = %.3g)" % (which, B, H, Wd, setting, name, err, float(np.abs(b).max())))
        if not err <= BAR:
            worst.append((name, err))
    assert not worst, worst
    h3, w3 = H // 4, Wd // 4
    first3 = {n: c for n, c in rows.items() if n.endswith("_200to128_%dx%d" % (h3, w3))}      # 32 + 168 -> 128: occlusion, flow[, past flow]
    print("table %s %dx%dx%d %-12s level-3 first decoder layers: %s" % (which, B, H, Wd, setting, first3))
    assert sum(first3.values()) == (3 if past else 2), first3
    if tag:
        assert list(first3) == ["conv%s_200to128_%dx%d" % (tag, h3, w3)], first3
        inner = [n for n in rows if n.startswith("conv%s_128to96_" % tag)]                    # and every level's third decoder layer
        assert len(inner) == 5, (inner, sorted(rows))
    if setting in STRIDE2_TAGS:
        must, never = STRIDE2_TAGS[setting]
        for t in must:
            assert any(n.startswith("conv%s_64to96_" % t) for n in rows), (t, sorted(rows))
        for t in never:
            assert not any(n.startswith("conv%s_" % t) for n in rows), (t, sorted(rows))
    if setting.startswith("corr-"):
        # The row name does not carry the variant, and launch_warp_costvol runs variant 3 where warp_costvol_unit_supported refuses a
        # launch: that variants 5 and 7 themselves run here rests on that predicate holding at these sizes (C a multiple of 16 at every
        # level).  Variants 0, 1 and 3 have no such fallback.
        assert sum(c for n, c in rows.items() if n.startswith("warp_costvol_")) == 5


# ---- (b) every image warp against float64 on the GPU's own flow ----

def _pool64(a):
    return 0.25 * (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2])


def _warp64(img, flow, k2):
    """BilinearSamplerBHWD (getTopLeft: clamp, THEN floor; four taps; a tap past the border has weight 0) in float64.
    img B x 3 x h x w, flow B x 2 x h x w, displacement k2 * flow."""
    B, _, h, w = img.shape
    f = flow.astype(np.float64) * k2
    out = np.empty_like(img)
    for b in range(B):
        cx = np.clip(np.arange(w)[None, :] + f[b, 0], 0, w - 1)
        cy = np.clip(np.arange(h)[:, None] + f[b, 1], 0, h - 1)
        xl, yt = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
        wx, wy = 1 - (cx - xl), 1 - (cy - yt)
        xr, yb = np.minimum(xl + 1, w - 1), np.minimum(yt + 1, h - 1)
        inx, iny = (xl + 1 <= w - 1), (yt + 1 <= h - 1)
        for c in range(3):
            p = img[b, c]
            out[b, c] = (wx * wy * p[yt, xl] + (1 - wx) * wy * np.where(inx, p[yt, xr], 0.0)
                         + wx * (1 - wy) * np.where(iny, p[yb, xl], 0.0) + (1 - wx) * (1 - wy) * np.where(inx & iny, p[yb, xr], 0.0))
    return out


def _warp_tolerance(img, l):
    """The sampler forms its coordinate x + k2 * u in fp32: the product and the sum are each rounded to half an ulp of a number below
    the map's width (height), so a coordinate that the clamp lets through is off by at most one ulp of it; 1 - (c - floor c) adds half
    an ulp of 1.  The result is piecewise linear in the coordinate with slope <= the largest difference between neighbouring pixels
    (Dx, Dy).  The four weighted taps: two roundings for a weight product, one for the tap, three sums, all on numbers <= M = max |pixel|
    with weights that sum to 1: 6 half-ulps, taken as 4 ulp.  The pyramid under it: l - 3 poolings of three sums each (the division
    by 4 is exact) against exact float64 means: 1.5 ulp of M per level."""
    h, w = img.shape[-2:]
    dx = float(np.abs(np.diff(img, axis=-1)).max())
    dy = float(np.abs(np.diff(img, axis=-2)).max())
    big = float(np.abs(img).max())
    return dx * (float(np.spacing(np.float32(w))) + EPS) + dy * (float(np.spacing(np.float32(h))) + EPS) + (4 + 1.5 * (l - 3)) * EPS * big


@pytest.mark.parametrize("B,H,Wd", TABLE_SIZES)
@pytest.mark.parametrize("which", KINDS)
def test_image_warps_vs_float64_on_the_gpus_own_flow(which, B, H, Wd):
    """iws[f][l] = warp of frame f's image pyramid (average pooling of x, l - 3 times) by k2 * skip_ufs[l] (skip_ubfs[l] for frame 1
    of a Soft model), k2 = 20 (f - 2) / 2^(l-3) (pwc.lua:422-446): recomputed from the GPU's own flow tensor, so that the error of
    everything upstream is out of the comparison."""
    past = which == "soft"
    x, flat, exp, got = _table_case(which, B, H, Wd)
    D.assert_conditions(exp, past)
    bad = []
    for f in (1, 3):
        img = x[:, 3 * (f - 1):3 * f].astype(np.float64)
        for l in range(3, 8):
            if l > 3:
                img = _pool64(img)
            flow = got[D.table_index(past, l, "ubfs" if (past and f == 1) else "ufs")]
            k2 = 20.0 * (f - 2) / 2.0 ** (l - 3)
            ref = _warp64(img, flow, k2)
            a = got[D.table_index(past, l, "iw%d" % f)]
            assert a.shape == ref.shape
            err, tol = float(np.abs(a - ref).max()), _warp_tolerance(img, l)
            moved = float(np.abs(flow * k2).max())
            print("warp %s %dx%dx%d iws%d[%d] max|gpu - float64| = %.3g  tolerance %.3g  (moves <= %.2f px)" % (which, B, H, Wd, f, l, err, tol, moved))
            assert moved > 2.0
            if not err <= tol:
                bad.append((f, l, err, tol))
    assert not bad, bad


# ---- (c) the occlusion softmax ----

@pytest.mark.parametrize("B,H,Wd", TABLE_SIZES)
@pytest.mark.parametrize("which", KINDS)
def test_occlusion_softmax_structure_and_value(which, B, H, Wd):
    past = which == "soft"
    x, flat, exp, got = _table_case(which, B, H, Wd)
    D.assert_conditions(exp, past)
    for l in range(3, 8):
        i = D.table_index(past, l, "occs")
        a, b = got[i], exp[i]
        Bn, two, h, w = a.shape
        blocks = a.reshape(Bn, 2, h // 4, 4, w // 4, 4)
        assert (blocks == blocks[:, :, :, :1, :, :1]).all(), "level %d: not constant on aligned 4 x 4 blocks" % l   # two nearest x2
        s = a[:, 0].astype(np.float64) + a[:, 1].astype(np.float64)
        assert np.abs(s - 1.0).max() <= 2 * EPS, (l, float(np.abs(s - 1.0).max()))     # two quotients of one sum: 2 ulp of 1
        err = float(np.abs(a - b).max())
        assert err <= BAR, (l, err)
        for c in (0, 1):
            assert (a[:, c] >= THR).any() and (a[:, c] < THR).any(), "level %d plane %d holds one mask value only" % (l, c)


@pytest.mark.parametrize("which", KINDS)
def test_occlusion_softmax_saturates_like_the_oracle(which):
    """Logit differences past expf's fp32 underflow (exp(-103.98) rounds to 0): the probabilities there are exactly 0 and 1, everything
    is finite.  The oracle's logit difference d is not in its table where it saturates; a second oracle forward on the occlusion heads
    scaled by 2^-7 (exact in fp32: the last layer has no activation) gives d / 128 unsaturated.  Pixels with | |d| - 104 | < 0.05 are
    left to the 1e-3 bar alone: the GPU's logits differ from the oracle's by fp32 re-association, about 1e-6 of a few hundred."""
    past = which == "soft"
    B, H, Wd, spread = 1, 128, 192, 150.0
    x, flat, exp, got = _table_case(which, B, H, Wd, spread)
    D.assert_conditions(exp, past)            # a median of 0 keeps just under half of each plane over the threshold
    small = flat.copy()
    v = W.views(small, past)
    for l in range(3, 8):
        v["l%d.occ.conv6.w" % l] *= np.float32(2.0 ** -7)
        v["l%d.occ.conv6.b" % l] *= np.float32(2.0 ** -7)
    low = O.pwc_forward(x, small, past)
    for l in range(3, 8):
        i = D.table_index(past, l, "occs")
        a, b = got[i], exp[i]
        d = 128.0 * D.logit_difference(low[i])
        assert np.isfinite(d).all() and np.isfinite(a).all()
        hi, lo = d > 104.05, d < -104.05
        print("saturation %s level %d: d in %.1f .. %.1f, %.1f %% > 104, %.1f %% < -104" % (which, l, d.min(), d.max(), 100 * hi.mean(), 100 * lo.mean()))
        if l == 3:
            assert hi.mean() >= 0.10 and lo.mean() >= 0.10
        for sel, one, zero in ((hi, 1, 0), (lo, 0, 1)):
            assert (b[:, one][sel] == 1.0).all() and (b[:, zero][sel] == 0.0).all()      # the oracle
            assert (a[:, one][sel] == 1.0).all() and (a[:, zero][sel] == 0.0).all(), "level %d" % l
        assert float(np.abs(a - b).max()) <= BAR
    for name, a, b in zip(_names(past), got, exp):
        assert float(np.abs(a - b).max()) <= BAR, name


# ---- (d) the three-output paths ----

def _clip(r, T, H0, W0):
    """T frames in [0, 1] with structure: a smooth scene that moves by (1, 3) pixels per frame, plus noise; T x 3 x H0 x W0"""
    base = r.random((3, H0 + T, W0 + 3 * T))
    k = np.ones(5) / 5
    for ax in (1, 2):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, base)
    frames = [base[:, T - 1 - t:T - 1 - t + H0, 3 * (T - 1 - t):3 * (T - 1 - t) + W0] for t in range(T)]
    return np.stack([np.clip(a + (r.random((3, H0, W0)) - 0.5) * 0.04, 0, 1).astype(np.float32) for a in frames])


def _images(seed, n, H0, W0):
    """n independent triplets: im1, im2, im3, each n x 3 x H0 x W0"""
    r = np.random.default_rng(seed)
    clips = [_clip(r, 3, H0, W0) for _ in range(n)]
    return [np.ascontiguousarray(np.stack([c[f] for c in clips])) for f in range(3)]


def _net_input(im1, im2, im3):
    """what computeFlow feeds the network (back2future.lua:48-71), by the oracle: n x 9 x fh x fw"""
    n, _, H0, W0 = im1.shape
    fh, fw = H0 - H0 % 64, W0 - W0 % 64
    return np.stack([O.image_scale_bilinear(O.color_normalize(np.concatenate([im1[b], im2[b], im3[b]], 0)), fh, fw) for b in range(n)])


def _oracle_three(ims, flat, past):
    """per triplet: (flow f64, fwd, bwd, near-threshold map at H0 x W0 [2 planes]) by the oracle's computeFlow"""
    n, _, H0, W0 = ims[0].shape
    res = []
    for b in range(n):
        eflow, efo, ebo, fnet, onet = O.compute_flow(ims[0][b], ims[1][b], ims[2][b], flat, past, want_net=True)
        near = O.image_scale_simple((np.abs(onet - THR) < 1e-3).astype(np.uint8), H0, W0).astype(bool)
        res.append((eflow, efo, ebo, near, onet))
    return res


def _check_three(flow, fo, bo, e, what, both=True):
    eflow, efo, ebo, near, _ = e
    err = float(np.abs(flow.astype(np.float64) - eflow).max())
    print("three outputs %s: max|flow - oracle| = %.3g, |flow| <= %.3g, masks %.1f %% / %.1f %% set, %d + %d near the threshold"
          % (what, err, float(np.abs(eflow).max()), 100 * efo.mean(), 100 * ebo.mean(), int(near[1].sum()), int(near[0].sum())))
    assert err <= BAR, (what, err)
    assert ((fo != efo) & ~near[1:2]).sum() == 0, what
    assert ((bo != ebo) & ~near[0:1]).sum() == 0, what
    if both:
        for msk in (fo, bo):
            assert msk.min() == 0 and msk.max() == 1, "%s: a mask holds one value only" % what


def _calibrated(which, ims):
    past = which == "soft"
    x = _net_input(*ims)
    flat = D.displaced_weights(SEED, past, x, DISP, SPREAD)
    table = O.pwc_forward(x, flat, past)
    D.assert_conditions(table, past)
    return x, flat, table


@pytest.mark.parametrize("H0,W0", [(128, 192), (131, 259)])
@pytest.mark.parametrize("which", KINDS)
def test_compute_flow_vs_oracle(which, H0, W0):
    past = which == "soft"
    ims = _images(H0 + W0, 1, H0, W0)
    x, flat, table = _calibrated(which, ims)
    e = _oracle_three(ims, flat, past)[0]
    assert float(np.abs(e[0]).max()) * 20 > 2.0                  # the final flow is whole pixels (x 20: back2future.lua:77-84 leaves it unscaled)
    m = _model(which, flat)
    try:
        flow, fo, bo = m.computeFlow(ims[0][0], ims[1][0], ims[2][0])
    finally:
        m.close()
    assert flow.shape == (2, H0, W0) and flow.dtype == np.float64
    _check_three(flow, fo, bo, e, "computeFlow %s %dx%d" % (which, H0, W0))


@pytest.mark.parametrize("H0,W0", [(128, 192), (131, 259)])
@pytest.mark.parametrize("which", KINDS)
def test_batch_f32_and_occ_prob_vs_oracle(which, H0, W0):
    """computeFlowBatch(dtype=float32, occ_prob=True): occ_prob is skip_occs[3] of the oracle's table (for a Soft model the oracle's
    est[3], `onet`), nearest-rescaled with the index rule of image.scale 'simple'."""
    past = which == "soft"
    n = 2
    ims = _images(3 * H0 + W0, n, H0, W0)
    x, flat, table = _calibrated(which, ims)
    es = _oracle_three(ims, flat, past)
    occ_net = table[D.table_index(past, 3, "occs")]
    if past:
        for b in range(n):
            np.testing.assert_array_equal(occ_net[b], es[b][4])
    m = _model(which, flat)
    try:
        flow, fo, bo, occ = m.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True)
    finally:
        m.close()
    assert flow.dtype == np.float32 and occ.dtype == np.float32 and occ.shape == (n, 2, H0, W0)
    eocc = occ_net if (H0 % 64, W0 % 64) == (0, 0) else _nearest(occ_net, H0, W0)
    err = float(np.abs(occ - eocc).max())
    print("occ_prob %s %dx%d: max|gpu - oracle| = %.3g, range %.4g .. %.4g" % (which, H0, W0, err, float(occ.min()), float(occ.max())))
    assert err <= BAR
    for c in (0, 1):
        assert (occ[:, c] >= THR).any() and (occ[:, c] < THR).any()
    for b in range(n):
        _check_three(flow[b], fo[b], bo[b], es[b], "batch f32 %s %dx%d triplet %d" % (which, H0, W0, b))


@pytest.mark.parametrize("unit", [False, True], ids=["normalized", "unit"])
@pytest.mark.parametrize("which", KINDS)
def test_forward_device_vs_oracle(which, unit):
    """b2f_forward_device (flow, skip_occs[3], est3) on image input; est3 of a Hard model is iws[1][3], the full-resolution warp that
    reads the caller's input tensor (normalized on the fly for unit input)."""
    past = which == "soft"
    B, H, Wd = 2, 128, 192
    ims = _images(17 + unit, B, H, Wd)
    x, flat, table = _calibrated(which, ims)                     # x: the normalized triplets
    raw = np.ascontiguousarray(np.concatenate(ims, axis=1))      # B x 9 x H x W in [0, 1]
    d_in = torch.from_numpy(raw if unit else x).cuda()
    m = _model(which, flat)
    try:
        outs = _outs(m, B, H, Wd)
        _run_triplets(m, d_in, H, Wd, unit, outs)
        got = [o.cpu().numpy() for o in outs]
    finally:
        m.close()
    exp = [table[0], table[D.table_index(past, 3, "occs")], table[2]]
    for name, a, b in zip(("flow", "skip_occs[3]", "est3"), got, exp):
        err = float(np.abs(a - b).max())
        print("forward_device %s %s %-12s max|gpu - oracle| = %.3g" % (which, "unit" if unit else "normalized", name, err))
        assert a.shape == b.shape and err <= BAR, (name, err)


@pytest.mark.parametrize("kind", ["normalized", "unit", "u8"])
@pytest.mark.parametrize("which", KINDS)
def test_forward_sequence_device_vs_triplets_and_oracle(which, kind):
    """T = 5 frames: bit-identical to the triplet entry AND within the bar of the oracle, so that the sequence warp kernels
    (warp_input_seq_kernel<float>, <unsigned char>) run through the clamp on flows of whole pixels."""
    past = which == "soft"
    T, H, Wd = 5, 128, 192
    r = np.random.default_rng(40 + len(kind))
    if kind == "normalized":
        frames = r.standard_normal((T, 3, H, Wd)).astype(np.float32)
        x = np.concatenate([frames[:-2], frames[1:-1], frames[2:]], axis=1)
        seq_in, f32, in_kind = frames, frames, back2future.IN_NORMALIZED
    else:
        clip = _clip(r, T, H, Wd)
        by = np.round(clip * 255).astype(np.uint8)
        f32 = clip if kind == "unit" else by.astype(np.float32) / np.float32(255)       # correctly rounded k / 255, as image.load
        seq_in, in_kind = (f32, back2future.IN_UNIT) if kind == "unit" else (by, back2future.IN_U8)
        x = np.stack([back2future.normalize(np.concatenate([f32[b], f32[b + 1], f32[b + 2]], 0)) for b in range(T - 2)])
    flat = D.displaced_weights(SEED, past, x, DISP, SPREAD)
    table = O.pwc_forward(x, flat, past)
    D.assert_conditions(table, past)
    d_seq, d_f32 = torch.from_numpy(seq_in).cuda(), torch.from_numpy(f32).cuda()
    m = _model(which, flat)
    try:
        exp_t, got = _outs(m, T - 2, H, Wd), _outs(m, T - 2, H, Wd)
        _run_triplets(m, _triplets(d_f32), H, Wd, in_kind != back2future.IN_NORMALIZED, exp_t)
        _run_sequence(m, d_seq, T, H, Wd, in_kind, got)
        same = [torch.equal(a, b) for a, b in zip(got, exp_t)]
        got = [o.cpu().numpy() for o in got]
    finally:
        m.close()
    exp = [table[0], table[D.table_index(past, 3, "occs")], table[2]]
    for name, a, b in zip(("flow", "skip_occs[3]", "est3"), got, exp):
        err = float(np.abs(a - b).max())
        print("forward_sequence_device %s %-10s %-12s max|gpu - oracle| = %.3g" % (which, kind, name, err))
        assert a.shape == b.shape and err <= BAR, (name, err)
    assert all(same), "%s %s: sequence and triplet entries differ in outputs %s" % (which, kind, [i for i, ok in enumerate(same) if not ok])


@pytest.mark.parametrize("which", KINDS)
def test_host_sequence_and_two_replicas_equal_the_batch_that_matches_the_oracle(which, monkeypatch):
    """computeFlowSequence over several sub-batches and the two-replica b2f_multi forms: bit-identical to one context's
    computeFlowBatch, which is held against the oracle here, with masks that hold both values."""
    past = which == "soft"
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    T, H0, W0 = 7, 140, 200
    V = _clip(np.random.default_rng(43), T, H0, W0)
    ims = [np.ascontiguousarray(a) for a in (V[:-2], V[1:-1], V[2:])]
    x, flat, table = _calibrated(which, ims)
    es = _oracle_three(ims, flat, past)
    by = np.round(V * 255).astype(np.uint8)
    m = _model(which, flat)
    mm = back2future.MultiModel("random:%s:%d:2.0" % (which, SEED), n_gpus=2, devices=[0, 0])
    try:
        L = _lib.lib()
        _lib.check(L.b2f_set_weights(C.c_void_p(L.b2f_multi_context(mm._h, 0)), _lib.fptr(flat), flat.size))
        _lib.check(L.b2f_multi_rebroadcast(mm._h))
        sums = mm.weights_checksums()
        assert mm.n_gpus == 2 and sums[0] == sums[1]
        exp = m.computeFlowBatch(*ims)
        for b in range(T - 2):
            _check_three(exp[0][b], exp[1][b], exp[2][b], es[b], "batch %s %dx%d triplet %d" % (which, H0, W0, b))
        exp_u8 = m.computeFlowBatch(by[:-2], by[1:-1], by[2:])
        for msk in exp_u8[1:]:
            assert msk.min() == 0 and msk.max() == 1
        with m.options(host_subbatch_pixels=4 * H0 * W0):
            seq, seq_u8 = m.computeFlowSequence(V), m.computeFlowSequence(by)
        for what, got, ref in (("sequence", seq, exp), ("sequence u8", seq_u8, exp_u8), ("multi batch", mm.computeFlowBatch(*ims), exp),
                               ("multi sequence", mm.computeFlowSequence(V), exp), ("multi sequence u8", mm.computeFlowSequence(by), exp_u8)):
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b, err_msg="%s %s" % (which, what))
    finally:
        mm.close()
        m.close()
