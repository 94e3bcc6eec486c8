"""GPU parity tests proper: the HIP path (through the C ABI of libb2f.so) against the CPU
oracle on the same seeded inputs.  Tolerances are written next to each comparison; the
end-to-end bar is BASELINE.json's: max-abs <= 1e-3 on flow / occlusion probabilities."""
import numpy as np
import pytest

from back2future_amd import back2future, ops, weights as W
from oracle import oracle as O
from tests.displaced import set_flow_bias

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def soft():
    m = back2future.Model("random:soft:5:2.0")
    yield m
    m.close()


def _need_experiments(m):
    """Kernels that were measured no faster than the defaults live in tools/experiments/csrc and are not in the product library;
    `python -m back2future_amd.build --experiments` builds libb2f_exp.so with them (run the suite with B2F_LIB=<that file>)."""
    if not m.get_option("experiments"):
        pytest.skip("experiment kernel: not in the product library (python -m back2future_amd.build --experiments; B2F_LIB=back2future_amd/libb2f_exp.so)")


def _rng(seed):
    return np.random.default_rng(seed)


def test_native_library_is_loaded(hard):
    import os
    from back2future_amd import _lib
    assert os.path.exists(_lib.SO_PATH)
    with open("/proc/self/maps") as f:
        assert os.path.basename(_lib.SO_PATH) in f.read()     # libb2f.so, or the experiments build named by B2F_LIB
    if not os.environ.get("B2F_LIB"):
        assert os.path.basename(_lib.SO_PATH) == "libb2f.so" and not hard.get_option("experiments")
    assert hard.n_params == 7193316 and not hard.past_flow


def test_weights_roundtrip(hard):
    w = W.random_init(5, False, 2.0)
    np.testing.assert_array_equal(hard.get_weights(), w)     # same generator on both sides, bit exact


@pytest.mark.parametrize("ci,co,stride,h,w,leaky", [
    (3, 16, 2, 64, 96, True), (16, 16, 1, 32, 48, True), (32, 64, 2, 24, 40, True), (96, 96, 1, 9, 30, True),
    (128, 192, 2, 8, 14, True), (192, 192, 1, 4, 7, True), (196, 128, 1, 16, 33, True), (32, 2, 1, 20, 17, False),
    (5, 7, 1, 3, 5, False), (64, 32, 1, 1, 2, True), (64, 64, 1, 40, 70, True), (8, 68, 1, 18, 34, False),
    (128, 128, 1, 33, 65, True), (16, 16, 1, 5, 37, False), (16, 16, 1, 35, 66, True), (32, 2, 1, 33, 18, True),
    (40, 32, 1, 17, 33, True), (24, 96, 1, 20, 40, True), (16, 32, 2, 24, 40, True), (16, 32, 2, 9, 33, False),
    (16, 32, 2, 7, 131, True), (16, 32, 2, 1, 1, True), (16, 32, 2, 18, 64, False), (12, 32, 2, 10, 12, True)])
def test_conv3x3(hard, ci, co, stride, h, w, leaky):
    r = _rng(ci * 1000 + co)
    x = r.standard_normal((2, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    got = ops.conv3x3(hard, x, wt, b, stride, leaky)
    exp = O.conv3x3(x, wt, b, stride, leaky)
    assert got.shape == exp.shape
    if stride == 1 and co >= 32 and co % 4 == 0 and not (ci == 16 and co == 16):
        # Winograd F(4x4,3x3): fp32 throughout, but the transforms (coefficients up to 8) amplify rounding:
        # measured <= 6e-5 absolute on these unit-variance outputs, mean error 1e-6
        np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1.5e-4)
        assert np.abs(got - exp).mean() < 5e-6
    else:
        # fp32 MFMA is an exact fmaf chain; only the summation order differs from the oracle
        np.testing.assert_allclose(got, exp, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("ci,co,h,w", [(128, 128, 16, 30), (96, 64, 9, 17), (40, 96, 33, 20), (264, 128, 8, 16), (64, 68, 7, 9)])
def test_conv3x3_f2x2_one_n_tile_per_block(hard, ci, co, h, w):
    """The F(2x2) kernel launched with one block per 32-output N tile (what small launches of wide layers use)."""
    r = _rng(ci + co)
    x = r.standard_normal((3, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    with hard.options(op_wino_split=1):
        got = ops.conv3x3(hard, x, wt, b, 1, True)
    np.testing.assert_allclose(got, O.conv3x3(x, wt, b, 1, True), rtol=2e-5, atol=3e-5)


@pytest.mark.parametrize("ci,co,h,w,blocks", [(128, 128, 40, 70, 3), (200, 128, 33, 65, 5), (32, 64, 17, 100, 2), (104, 192, 48, 33, 7),
                                              (64, 100, 70, 31, 64), (40, 160, 16, 32, 2), (32, 32, 49, 35, 5), (128, 96, 36, 83, 17), (64, 32, 20, 70, 3)])
def test_conv3x3_wino4_persistent_blocks(hard, ci, co, h, w, blocks):
    """The persistent form of the F(4x4) kernel (one block walks several tiles, the K pipeline runs across tile boundaries):
    forced with a given number of blocks at test sizes -- odd and even chunk counts, ragged edges, one to many tiles per
    block -- against the oracle and, bit for bit, against the one-tile-per-block kernel (the launcher picks between them by
    launch size, and batching must not change a bit)."""
    r = _rng(ci * 7 + co + blocks)
    x = r.standard_normal((3, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    with hard.options(wino4_persistent=0):
        one_tile = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino4_persistent=blocks):   # values > 1: exactly that many persistent blocks
        got = ops.conv3x3(hard, x, wt, b, 1, True)
    exp = O.conv3x3(x, wt, b, 1, True)
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1.5e-4)
    assert np.abs(got - exp).mean() < 5e-6
    assert np.array_equal(got, one_tile)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
@pytest.mark.parametrize("ci,co,h,w,blocks", [(128, 128, 40, 70, 3), (200, 128, 33, 65, 5), (32, 64, 17, 100, 2), (104, 192, 48, 33, 7),
                                              (64, 100, 70, 31, 64), (96, 160, 16, 32, 2)])
def test_conv3x3_wino4_split_operands(hard, scale, ci, co, h, w, blocks):
    """Option wino4_split = 1: the F(4x4) GEMMs on the bf16 matrix pipe with every fp32 operand split exactly into three bf16
    terms, six of the nine term products kept (b2f_wino4s.hip).  The claim is fp32-level accuracy: against an fp64 convolution
    its error must stay inside the fp32-MFMA kernel's own bars (the same atol / mean bars as test_conv3x3, in proportion to
    the activation scale) and within 1.25x of the fp32 kernel's measured error on the same case; and the bits must not depend
    on how many persistent blocks walk the tiles."""
    import torch
    _need_experiments(hard)
    r = _rng(ci * 11 + co + blocks)
    x = (r.standard_normal((3, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = (r.standard_normal(co, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(wino4_persistent=blocks, wino4_split=0):
        f32 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino4_persistent=blocks, wino4_split=1):
        got = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino4_persistent=1, wino4_split=1):
        got1 = ops.conv3x3(hard, x, wt, b, 1, True)
    assert not np.array_equal(got, f32)                      # the other kernel really ran
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert es.max() <= 1.5e-4 * scale and es.mean() < 5e-6 * scale
    assert es.mean() <= 1.25 * ef.mean() and es.max() <= 1.25 * ef.max() + 1e-5 * scale
    assert np.array_equal(got, got1)


@pytest.mark.parametrize("k", [3, 4, 9])
def test_conv3x3_wino4_hybrid_steps(hard, k):
    """Option wino4_hybrid = k: k of a wave's nine xi steps of the persistent F(4x4) kernel on the bf16 pipe with split operands,
    the others on the fp32 MFMA (an experiment kept as an option: measured no faster).  Same accuracy claim as wino4_split."""
    import torch
    _need_experiments(hard)
    ci, co, h, w = 200, 128, 33, 65
    r = _rng(900 + k)
    x = r.standard_normal((2, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(wino4_persistent=5):
        f32 = ops.conv3x3(hard, x, wt, b, 1, True)
        with hard.options(wino4_hybrid=k):
            got = ops.conv3x3(hard, x, wt, b, 1, True)
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert not np.array_equal(got, f32)
    assert es.max() <= 1.5e-4 and es.mean() < 5e-6 and es.mean() <= 1.25 * ef.mean()


@pytest.mark.parametrize("scale", [1e-3, 30.0, 1e3])
@pytest.mark.parametrize("ci,co,h,w", [(128, 128, 33, 65), (200, 96, 40, 70)])
def test_conv3x3_wino4_activation_scale(hard, scale, ci, co, h, w):
    """The F(4x4) transforms (coefficients up to 8) amplify fp32 rounding RELATIVE to the activations: the error bar of
    test_conv3x3 must hold in proportion at any activation scale (trained models see activations far from unit variance)."""
    r = _rng(int(ci + co + scale))
    x = (r.standard_normal((2, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = (r.standard_normal(co, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    for persistent in (0, 3):
        with hard.options(wino4_persistent=persistent):
            got = ops.conv3x3(hard, x, wt, b, 1, True)
        exp = O.conv3x3(x, wt, b, 1, True)
        np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1.5e-4 * scale)
        assert np.abs(got - exp).mean() < 5e-6 * scale


def test_conv3x3_transpose_detecting(hard):
    """asymmetric single-tap kernels: catches swapped rows/cols, taps or channels."""
    x = np.arange(2 * 8 * 6 * 10, dtype=np.float32).reshape(2, 8, 6, 10) / 100
    for (ky, kx, ci, co) in [(0, 2, 3, 5), (2, 0, 7, 1), (1, 1, 0, 30)]:
        wt = np.zeros((33, 8, 3, 3), np.float32)
        wt[co, ci, ky, kx] = 1
        got = ops.conv3x3(hard, x, wt, np.zeros(33, np.float32), 1, False)
        # stride-1 layers run on the Winograd kernel: same values up to fp32 re-association of the transforms
        np.testing.assert_allclose(got, O.conv3x3(x, wt, np.zeros(33, np.float32), 1, False), rtol=0, atol=4e-6)
    # the same through the F(4x4) kernel (>= 64 outputs), 16 x 32-pixel blocks with ragged edges
    x = (np.arange(2 * 8 * 21 * 37, dtype=np.float32).reshape(2, 8, 21, 37) % 97) / 50
    for (ky, kx, ci, co) in [(0, 2, 3, 5), (2, 0, 7, 65), (1, 1, 0, 30), (2, 2, 5, 67)]:
        wt = np.zeros((68, 8, 3, 3), np.float32)
        wt[co, ci, ky, kx] = 1
        got = ops.conv3x3(hard, x, wt, np.zeros(68, np.float32), 1, False)
        np.testing.assert_allclose(got, O.conv3x3(x, wt, np.zeros(68, np.float32), 1, False), rtol=0, atol=2e-5)


@pytest.fixture(params=[0, 1, 2, 3, 4, 5, 6, 7, 8], ids=["corr-regular", "corr-latency", "corr-two-pixel", "corr-two-pixel-one-direction", "corr-window-staged", "corr-unit", "corr-roles", "corr-sixteen-waves", "corr-four-pixel"])
def corr_variant(request, hard):
    """Every instantiation of the warp + cost-volume kernel (the launcher would pick by map / launch size; variants 5 and 6, the
    persistent unit kernel and its role-specialised form, serve channel counts that are multiples of 16 and hand the others to
    variant 3).  Variants 2, 4, 6 and 8 are experiments (tools/experiments): they run with the experiments build only."""
    if request.param in (2, 4, 6, 8):
        _need_experiments(hard)
    with hard.options(corr_variant=request.param):
        yield request.param


@pytest.mark.parametrize("C,h,w", [(32, 24, 40), (192, 4, 7), (96, 9, 17), (8, 1, 2), (64, 16, 16)])
def test_costvol_no_warp(hard, corr_variant, C, h, w):
    r = _rng(C + h)
    ref = r.standard_normal((2, C, h, w), dtype=np.float32)
    frm = r.standard_normal((2, C, h, w), dtype=np.float32)
    for fwd in (True, False):
        got = ops.costvol(hard, ref, frm, 9, fwd)
        exp = O.costvol([ref, frm], 9, fwd)
        np.testing.assert_allclose(got, exp, rtol=1e-5, atol=2e-6)


def test_costvol_generic_window(hard):
    r = _rng(3)
    ref = r.standard_normal((1, 6, 11, 13), dtype=np.float32)
    frm = r.standard_normal((1, 6, 11, 13), dtype=np.float32)
    for win in (5, 3):
        for fwd in (True, False):
            np.testing.assert_allclose(ops.costvol(hard, ref, frm, win, fwd), O.costvol([ref, frm], win, fwd),
                                       rtol=1e-5, atol=2e-6)


def test_costvol_impulse_known_answer(hard):
    """CostVolMulti.lua:225-254: a point moving (+1,+1) per frame lights channel
    (-1+4)*9 + (-1+4) in both volumes."""
    h = w = 16
    prev = np.zeros((1, 8, h, w), np.float32); cur = prev.copy(); nxt = prev.copy()
    prev[0, 0, 4, 5] = 8; cur[0, 0, 5, 6] = 1; nxt[0, 0, 6, 7] = 8
    cv = ops.warp_costvol(hard, cur, nxt, prev, None, 0.0)
    c = 3 * 9 + 3
    assert cv[0, c, 5, 6] == 1 and cv[0, 81 + c, 5, 6] == 1
    assert cv[0, :81].sum() == 1 and cv[0, 81:].sum() == 1


@pytest.mark.parametrize("C,h,w,k", [(32, 24, 40, 2.5), (128, 8, 14, 0.625), (64, 16, 30, 5.0)])
def test_warp_costvol_fused(hard, corr_variant, C, h, w, k):
    """fused kernel == warpingUnit x2 + CostVolMulti x2 + JoinTable of the oracle."""
    r = _rng(C * 7 + h)
    ref = r.standard_normal((2, C, h, w), dtype=np.float32)
    f3 = r.standard_normal((2, C, h, w), dtype=np.float32)
    f1 = r.standard_normal((2, C, h, w), dtype=np.float32)
    flow = (r.standard_normal((2, 2, h, w)) * 0.8).astype(np.float32)
    flow[0, :, 0, 0] = (-30, -30); flow[0, :, 1, 1] = (30, 30)      # force the border clamp
    got = ops.warp_costvol(hard, ref, f3, f1, flow, k)
    w3 = O.warping_unit(f3, flow, k)
    w1 = O.warping_unit(f1, flow, -k)
    exp = np.concatenate([O.costvol([ref, w3], 9, True), O.costvol([ref, w1], 9, False)], 1)
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=5e-6)


@pytest.mark.parametrize("C,B,h,w,k,scale", [(32, 3, 145, 456, 0.3125, 1.0), (64, 2, 70, 130, 5.0, 8.0), (96, 2, 33, 65, 2.5, 0.1), (192, 3, 16, 30, 0.625, 1.0),
                                              (128, 1, 9, 17, 1.25, 8.0), (48, 2, 24, 40, 2.5, 1.0), (16, 1, 1, 2, 1.25, 0.0),
                                              (32, 2, 60, 200, 0.625, -1.0), (64, 1, 40, 90, 1.25, -1.0)])
@pytest.mark.parametrize("variant", [5, 6, 7, 8])
def test_warp_costvol_unit_kernel_bit_identical(hard, variant, C, B, h, w, k, scale):
    """The persistent unit kernel (corr_variant 5: many tile-directions per block, 16-channel stages, ragged tiles, flows through
    the border clamp, no flow at all), its sixteen-wave form (7: ten unit waves + six gather waves) and its role-specialised form (6: FMA waves / gather waves, source window by LDS-DMA where a
    tile-direction's taps fit it -- scale -1: a translation + small noise, the smooth case that takes the window; white-noise flows
    take its gather fallback) compute the bits of the two-pixel kernel (variant 3) -- same operations in the same order."""
    if variant in (6, 8):
        _need_experiments(hard)
    r = _rng(C * 31 + h)
    ref = r.standard_normal((B, C, h, w), dtype=np.float32)
    f3 = r.standard_normal((B, C, h, w), dtype=np.float32)
    f1 = r.standard_normal((B, C, h, w), dtype=np.float32)
    flow = None if scale == 0.0 else (r.standard_normal((B, 2, h, w)) * scale).astype(np.float32)
    if scale < 0:
        flow = (r.uniform(-6, 6, (B, 2, 1, 1)) + 0.15 * r.standard_normal((B, 2, h, w))).astype(np.float32)
    with hard.options(corr_variant=3):
        a = ops.warp_costvol(hard, ref, f3, f1, flow, k)
    with hard.options(corr_variant=variant):
        b = ops.warp_costvol(hard, ref, f3, f1, flow, k)
    assert np.abs(a).max() > 0
    np.testing.assert_array_equal(a, b)


def test_warp_bhwd(hard):
    r = _rng(11)
    img = r.standard_normal((2, 9, 12, 5), dtype=np.float32)
    grid = (r.standard_normal((2, 9, 12, 2)) * 3).astype(np.float32)
    grid[0, 0, 0] = (-50, -50); grid[0, 1, 1] = (50, 50); grid[0, 2, 2] = (0, 0)
    np.testing.assert_allclose(ops.warp_bhwd(hard, img, grid), O.warp_bhwd(img, grid), rtol=1e-5, atol=1e-6)
    zero = np.zeros_like(grid)
    np.testing.assert_array_equal(ops.warp_bhwd(hard, img, zero), img)      # zero flow = identity
    g2 = np.zeros((2, 4, 6, 2), np.float32)                                   # the grid sizes the output
    np.testing.assert_array_equal(ops.warp_bhwd(hard, img, g2), O.warp_bhwd(img, g2))


def test_upsample_flow(hard):
    r = _rng(5)
    for (h, w) in [(6, 9), (1, 3), (16, 30)]:
        x = r.standard_normal((2, 2, h, w), dtype=np.float32)
        np.testing.assert_allclose(ops.upsample_flow2x(hard, x), O.upsample_bilinear2x(x), rtol=1e-5, atol=1e-6)


def _triplet(r, H, W):
    """smooth image + shifted copies, so that the flow decoders see real structure."""
    base = r.random((3, H + 16, W + 16)).astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for ax in (1, 2):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, base).astype(np.float32)
    im1 = base[:, 8:8 + H, 8:8 + W]
    im2 = base[:, 7:7 + H, 5:5 + W]
    im3 = base[:, 6:6 + H, 2:2 + W]
    n = lambda: (r.random((3, H, W)).astype(np.float32) - 0.5) * 0.04
    return [np.clip(a + n(), 0, 1).astype(np.float32) for a in (im1, im2, im3)]


@pytest.mark.parametrize("which,H,Wd", [("hard", 128, 192), ("soft", 128, 192), ("soft", 64, 64), ("hard", 192, 320)])
def test_compute_flow_end_to_end(hard, soft, corr_variant, which, H, Wd):
    """computeFlow (flow, fwd_occ, bwd_occ) on a /64 input: HIP path vs oracle.
    Bar: max-abs(flow) <= 1e-3, EPE <= 1e-3 (BASELINE.json); masks may differ only where
    est[3] is within 1e-3 of the 0.6666 threshold."""
    m = hard if which == "hard" else soft
    r = _rng(H + Wd)
    im1, im2, im3 = _triplet(r, H, Wd)
    flow, fo, bo = m.computeFlow(im1, im2, im3)
    wflat = W.random_init(5, which == "soft", 2.0)
    eflow, efo, ebo, fnet, onet = O.compute_flow(im1, im2, im3, wflat, which == "soft", want_net=True)
    assert flow.shape == (2, H, Wd) and fo.shape == (1, H, Wd) and fo.dtype == np.uint8
    assert np.abs(eflow).max() > 0.02
    d = np.abs(flow - eflow)
    epe = np.sqrt(((flow - eflow) ** 2).sum(0)).mean()
    assert d.max() <= 1e-3 and epe <= 1e-3, (d.max(), epe)
    near = np.abs(onet - 0.6666) < 1e-3
    assert ((fo != efo) & ~near[1:2]).sum() == 0
    assert ((bo != ebo) & ~near[0:1]).sum() == 0


@pytest.mark.parametrize("which,H,Wd,bias", [("hard", 128, 192, (0.6, -0.4)), ("soft", 192, 320, (-0.5, 0.7)), ("hard", 128, 192, (3.0, 2.0))])
def test_compute_flow_large_displacements(which, H, Wd, bias):
    """Random weights give flows of a fraction of a pixel; trained models move features by many pixels.  Here the last layer of
    every flow decoder carries a bias, so every level predicts flow = bias + network term: the warps of the next level sample
    3 .. 15 pixels (level-3 units) away -- through the border clamp for a large part of the map at the coarse levels, and past
    the 32 x 32 window of the window-staged cost-volume variant for the largest bias (its gather fallback).  Same bar as the
    other end-to-end tests, on every cost-volume instantiation."""
    past = which == "soft"
    flat = W.random_init(7, past, 1.0)
    set_flow_bias(flat, past, bias)
    r = _rng(H * 3 + Wd)
    im1, im2, im3 = _triplet(r, H, Wd)
    eflow, efo, ebo, fnet, onet = O.compute_flow(im1, im2, im3, flat, past, want_net=True)
    assert np.abs(eflow).max() > 0.3
    m = back2future.Model("random:%s:7:1.0" % which)
    try:
        m.set_weights(flat)
        for variant in (-1, 0, 3, 4, 5, 6, 7):
            if variant in (4, 6) and not m.get_option("experiments"):
                continue
            with m.options(corr_variant=variant):
                flow, fo, bo = m.computeFlow(im1, im2, im3)
            d = np.abs(flow - eflow)
            epe = np.sqrt(((flow - eflow) ** 2).sum(0)).mean()
            assert d.max() <= 1e-3 and epe <= 1e-3, (variant, d.max(), epe)
            near = np.abs(onet - 0.6666) < 1e-3
            assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0
    finally:
        m.close()


@pytest.mark.parametrize("min_px,adaptive", [(0, 0), (1000000, 0), (4096, 1)])
def test_compute_flow_either_winograd_kernel(hard, min_px, adaptive):
    """The launcher picks F(4x4) or F(2x2) per map size, which at test sizes means F(2x2) for most layers: force every
    eligible layer of the graph onto the F(4x4) kernel (wino4_min_pixels = 0) and onto F(2x2) (1e6); the third case
    is the opt-in per-launch rule (block rounds on the chip)."""
    r = _rng(12)
    H, Wd = 128, 256
    ims = _triplet(r, H, Wd)
    with hard.options(wino4_min_pixels=min_px, adaptive_kernels=adaptive, host_graph=0):
        flow, fo, bo = hard.computeFlow(*ims)
    eflow, efo, ebo, fnet, onet = O.compute_flow(*ims, W.random_init(5, False, 2.0), False, want_net=True)
    d = np.abs(flow - eflow)
    assert np.abs(eflow).max() > 0.02 and d.max() <= 1e-3, d.max()
    near = np.abs(onet - 0.6666) < 1e-3
    assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0


def test_compute_flow_with_split_operand_winograd(hard):
    """The whole graph with every two-N-tile F(4x4) launch on the bf16 matrix pipe (option wino4_split, split fp32 operands):
    same end-to-end bar as the default path; the option repacks the weights when it is switched and back."""
    _need_experiments(hard)
    r = _rng(14)
    H, Wd = 128, 256
    ims = _triplet(r, H, Wd)
    eflow, efo, ebo, fnet, onet = O.compute_flow(*ims, W.random_init(5, False, 2.0), False, want_net=True)
    with hard.options(wino4_min_pixels=0, adaptive_kernels=0, host_graph=0):
        base, _, _ = hard.computeFlow(*ims)
        with hard.options(wino4_split=1):
            flow, fo, bo = hard.computeFlow(*ims)
        again, _, _ = hard.computeFlow(*ims)
    d = np.abs(flow - eflow)
    assert np.abs(eflow).max() > 0.02 and d.max() <= 1e-3, d.max()
    assert not np.array_equal(flow, base) and np.abs(flow - base).max() < 1e-5     # another kernel, the same function
    assert np.array_equal(again, base)
    near = np.abs(onet - 0.6666) < 1e-3
    assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
@pytest.mark.parametrize("B,h,w", [(1, 32, 60), (2, 37, 71), (3, 5, 9), (1, 130, 61), (1, 256, 64), (2, 16, 300)])
def test_fused_head_on_the_bf16_pipe(hard, scale, B, h, w):
    """b2f_op_conv_head16 = the kernel the default pipeline (option bf16_direct = 2) runs for conv(16,16,s1)+LeakyReLU -> conv(16,32,s2)+
    LeakyReLU (pwc.lua:60-62): one streaming kernel, split fp32 operands on the bf16 matrix pipe, the 16-channel map kept in LDS.
    Checked against the oracle's two convolutions and an fp64 reference: fp32-level accuracy (inside the bars of test_conv3x3 and
    within 1.5x of the chained fp32-MFMA kernels' own error), strips / row blocks / odd sizes / image borders included."""
    import torch
    r = _rng(B * 1000 + h * 7 + w)
    x = (r.standard_normal((B, 16, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    w1 = (r.standard_normal((16, 16, 3, 3), dtype=np.float32) / 12).astype(np.float32)
    w2 = (r.standard_normal((32, 16, 3, 3), dtype=np.float32) / 12).astype(np.float32)
    b1 = (r.standard_normal(16, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    b2 = (r.standard_normal(32, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    t = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w1).double(), torch.from_numpy(b1).double(), padding=1)
    t = torch.where(t > 0, t, 0.2 * t)
    t = torch.nn.functional.conv2d(t, torch.from_numpy(w2).double(), torch.from_numpy(b2).double(), padding=1, stride=2)
    exp = torch.where(t > 0, t, 0.2 * t).numpy()
    got = ops.conv_head16(hard, x, w1, b1, w2, b2)
    with hard.options(bf16_direct=0):
        f32 = ops.conv3x3(hard, ops.conv3x3(hard, x, w1, b1, 1, True), w2, b2, 2, True)
    ora = O.conv3x3(O.conv3x3(x, w1, b1, 1, True), w2, b2, 2, True)
    assert got.shape == exp.shape and np.isfinite(got).all()
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert es.max() <= 1e-4 * scale and es.mean() < 5e-6 * scale
    assert es.max() <= 1.5 * ef.max() + 1e-6 * scale
    assert np.abs(got - ora).max() <= 1e-4 * scale


@pytest.mark.parametrize("B,h,w", [(1, 16, 32), (2, 37, 70), (3, 64, 33)])
def test_conv16_on_the_bf16_pipe(hard, B, h, w):
    """Option bf16_direct = 1: the 16 -> 16 layer alone on the bf16 pipe (b2f_conv16b.hip), same accuracy claim."""
    import torch
    _need_experiments(hard)
    r = _rng(B * 77 + h + w)
    x = r.standard_normal((B, 16, h, w), dtype=np.float32)
    wt = (r.standard_normal((16, 16, 3, 3), dtype=np.float32) / 12).astype(np.float32)
    b = r.standard_normal(16, dtype=np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(bf16_direct=0):
        f32 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(bf16_direct=1):
        got = ops.conv3x3(hard, x, wt, b, 1, True)
    assert not np.array_equal(got, f32)
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert es.max() <= 1e-4 and es.max() <= 1.5 * ef.max() + 1e-6


@pytest.mark.parametrize("B,ci,co,h,w,stride,scale", [(1, 32, 64, 16, 64, 2, 1.0), (2, 32, 64, 37, 71, 2, 1.0), (1, 64, 96, 33, 50, 2, 300.0), (3, 96, 128, 9, 130, 2, 1e-3),
                                                      (1, 128, 192, 32, 60, 2, 1.0), (2, 40, 64, 20, 20, 2, 1.0), (1, 64, 100, 31, 33, 2, 1.0), (1, 24, 32, 40, 66, 2, 1.0),
                                                      (1, 64, 32, 40, 66, 1, 1.0)])
def test_direct_conv_on_the_bf16_pipe(hard, B, ci, co, h, w, stride, scale):
    """Option bf16_conv = 1 (the default for the stride-2 layers of the pyramid, pwc.lua:60): the direct implicit-GEMM kernel with split
    fp32 operands on the bf16 matrix pipe (b2f_convb.hip) against an fp64 convolution and the fp32-MFMA direct kernel: fp32-level
    accuracy (inside test_conv3x3's bars, within 1.5x of the fp32 kernel's own error); whole blocks of 64 outputs + a 32-output
    remainder launch, odd sizes, borders, two output tiles per wave."""
    import torch
    r = _rng(ci * 13 + co + h)
    x = (r.standard_normal((B, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = (r.standard_normal(co, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1, stride=stride)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(bf16_conv=0):
        f32 = ops.conv3x3(hard, x, wt, b, stride, True)
    with hard.options(bf16_conv=2, bf16_conv_min_pixels=0):
        got = ops.conv3x3(hard, x, wt, b, stride, True)
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert np.isfinite(got).all() and not np.array_equal(got, f32)
    assert es.max() <= 1e-4 * scale and es.mean() < 5e-6 * scale
    assert es.max() <= 1.5 * ef.max() + 1e-6 * scale


def test_compute_flow_head_kernels_agree(hard):
    """The whole graph with the head of the pyramid on the fp32-MFMA kernels (bf16_direct = 0), with the 16 -> 16 layer on the bf16 pipe
    (1) and with the fused head (2, the default): the same function within fp32 rounding, each inside the end-to-end bar."""
    r = _rng(21)
    H, Wd = 128, 256
    ims = _triplet(r, H, Wd)
    eflow, efo, ebo, fnet, onet = O.compute_flow(*ims, W.random_init(5, False, 2.0), False, want_net=True)
    flows = {}
    opts = (0, 1, 2) if hard.get_option("experiments") else (0, 2)        # 1 = an experiment kernel (tools/experiments)
    for o in opts:
        with hard.options(bf16_direct=o, host_graph=0):
            flows[o], _, _ = hard.computeFlow(*ims)
        assert np.abs(flows[o] - eflow).max() <= 1e-3
    assert hard.get_option("bf16_direct") == 2
    assert not np.array_equal(flows[0], flows[2]) and np.abs(flows[0] - flows[2]).max() < 2e-5
    if 1 in flows:
        assert np.abs(flows[0] - flows[1]).max() < 2e-5


def test_compute_flow_non_multiple_of_64(soft):
    """375 x 1242-style input: host-side image.scale to 320 x 1216-style size, nearest rescale back."""
    r = _rng(77)
    H0, W0 = 150, 200                          # -> 128 x 192 net size
    im1, im2, im3 = _triplet(r, H0, W0)
    flow, fo, bo = soft.computeFlow(im1, im2, im3)
    wflat = W.random_init(5, True, 2.0)
    eflow, efo, ebo, fnet, onet = O.compute_flow(im1, im2, im3, wflat, True, want_net=True)
    assert flow.shape == (2, H0, W0)
    assert np.abs(flow - eflow).max() <= 1e-3
    near = O.image_scale_simple((np.abs(onet - 0.6666) < 1e-3).astype(np.uint8), H0, W0).astype(bool)
    assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0


@pytest.mark.parametrize("Hs,Ws,Hd,Wd", [(150, 200, 128, 192), (375, 1242, 320, 1216), (70, 64, 64, 64), (64, 90, 64, 64),
                                         (40, 50, 64, 80), (33, 1, 48, 5), (64, 64, 64, 64), (97, 131, 13, 17)])
@pytest.mark.parametrize("normalize", [False, True])
def test_image_scale_bit_exact(hard, Hs, Ws, Hd, Wd, normalize):
    """image.scale 'bilinear' (+ ColorNormalize) on the device vs the CPU routine: same IEEE operations in the
    same order, so not one bit may differ (down, up, mixed and identity axes)."""
    r = _rng(Hs * 7 + Wd)
    src = r.random((9, Hs, Ws)).astype(np.float32)
    exp = O.image_scale_bilinear(O.color_normalize(src) if normalize else src, Hd, Wd)
    got = ops.image_scale(hard, src, Hd, Wd, normalize)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_color_normalize_is_the_ieee_quotient(hard):
    """The device ColorNormalize forms (x - mean) / std without a float division (scaled Markstein correction step,
    b2f_internal.h:color_normalize; tools/div_const_check.hip proves it for every float32 on the GPU): same bits as numpy's
    division on pixel values, on every float32 neighbour of the means, on huge, tiny, infinite and NaN inputs."""
    r = _rng(77)
    mean = np.array([0.485, 0.456, 0.406], np.float32)
    near = np.concatenate([np.nextafter(np.full(40, m, np.float32), np.float32(d)) for m in mean for d in (0, 1)])
    for k in range(1, 40):
        near[k::40] = np.nextafter(near[k - 1::40], np.float32(1) if k % 2 else np.float32(0))
    special = np.array([0, -0.0, 1, 1e-45, -1e-45, 1e-38, 3e38, -3e38, 7.7e37, -7.7e37, 7.8e37, 3.4028235e38, np.inf, -np.inf, np.nan,
                        255, 1 / 255, 0.5, 2 ** -126, 1e20, -1e20], np.float32)
    wide = (r.standard_normal(4000) * np.exp(r.uniform(-80, 88, 4000))).astype(np.float32)
    vals = np.concatenate([r.random(9 * 64 * 64 - near.size - special.size - wide.size).astype(np.float32), near, special, wide])
    src = r.permutation(vals).reshape(9, 64, 64)
    with np.errstate(all="ignore"):
        exp = O.color_normalize(src)
    got = ops.image_scale(hard, src, 64, 64, True)           # identity scale: the normalization alone
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    np.testing.assert_array_equal(got.view(np.uint32)[ok], exp.view(np.uint32)[ok])


@pytest.mark.parametrize("which,H0,W0", [("soft", 150, 200), ("hard", 131, 259)])
def test_compute_flow_boundary_bit_exact(hard, soft, which, H0, W0):
    """The device pre/post-processing of computeFlow (back2future.lua:48-93) around the network: feed model:forward
    the CPU-prepared input, post-process its est[1] / est[3] on the CPU, and require computeFlow's results to be
    bit-identical (flow in f64, masks)."""
    m = hard if which == "hard" else soft
    r = _rng(H0 + W0)
    ims = _triplet(r, H0, W0)
    fh, fw = H0 - H0 % 64, W0 - W0 % 64
    x = O.image_scale_bilinear(O.color_normalize(np.concatenate(ims, 0)), fh, fw)[None]
    outs = m.forward(x)
    fnet, est3 = outs[0][0].astype(np.float64), outs[2][0].astype(np.float64)
    eflow = O.image_scale_simple(fnet, H0, W0)
    eflow[0] *= float(W0) / float(fw)
    eflow[1] *= float(H0) / float(fh)
    eocc = O.image_scale_simple(est3, H0, W0)
    flow, fo, bo = m.computeFlow(*ims)
    np.testing.assert_array_equal(flow, eflow)
    np.testing.assert_array_equal(fo[0], (eocc[1] >= 0.6666).astype(np.uint8))
    np.testing.assert_array_equal(bo[0], (eocc[0] >= 0.6666).astype(np.uint8))


def test_host_pipeline_many_sub_batches(soft):
    """b2f_compute_flow_batch cut into one-triplet sub-batches (5 of them through the two buffer sets, pageable
    and page-locked caller buffers): every triplet must equal its stand-alone computeFlow bit for bit."""
    import torch
    r = _rng(31)
    H0, W0, n = 70, 140, 5
    trip = [_triplet(r, H0, W0) for _ in range(n)]
    im = [np.stack([t[i] for t in trip]) for i in range(3)]
    single = [soft.computeFlow(*t) for t in trip]
    with soft.options(host_subbatch_pixels=H0 * W0, host_threads=3):
        res = [soft.computeFlowBatch(*im)]
        pin_in = [torch.from_numpy(a).pin_memory() for a in im]
        pin_out = (torch.empty((n, 2, H0, W0), dtype=torch.float64).pin_memory(),
                   torch.empty((n, 1, H0, W0), dtype=torch.uint8).pin_memory(),
                   torch.empty((n, 1, H0, W0), dtype=torch.uint8).pin_memory())
        res.append(soft.computeFlowBatch(*[t.numpy() for t in pin_in], out=tuple(t.numpy() for t in pin_out)))
        soft.set_option("host_subbatch_pixels", 2 * H0 * W0)      # 2 + 2 + 1
        res.append(soft.computeFlowBatch(*im))
    for fb, fob, bob in res:
        for i in range(n):
            np.testing.assert_array_equal(fb[i], single[i][0])
            np.testing.assert_array_equal(fob[i], single[i][1])
            np.testing.assert_array_equal(bob[i], single[i][2])


@pytest.mark.parametrize("H0,W0", [(64, 128), (67, 131)])
def test_host_pipeline_8bit_transport_is_lossless(hard, H0, W0):
    """Inputs that are k / 255 (what image.load returns for 8-bit files) cross the link as bytes and are rebuilt on
    the device; the results must equal the float upload bit for bit -- also when a later triplet of the same call
    is not 8-bit data and the call falls back to floats from there on."""
    r = _rng(H0)
    n = 5
    q = lambda a: (np.round(a * 255.0).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    trip = [_triplet(r, H0, W0) for _ in range(n)]
    trip = [[q(a) for a in t] if i != 3 else t for i, t in enumerate(trip)]     # triplet 3 keeps arbitrary floats
    im = [np.stack([t[i] for t in trip]) for i in range(3)]
    hard.set_option("host_subbatch_pixels", 2 * H0 * W0)
    hard.set_option("host_u8", 0)
    ref = hard.computeFlowBatch(*im)
    ref4 = hard.computeFlowBatch(*[a[:3] for a in im])
    hard.set_option("host_u8", 1)
    got = hard.computeFlowBatch(*im)
    got4 = hard.computeFlowBatch(*[a[:3] for a in im])                          # all three triplets go as bytes
    for a, b in zip(ref + ref4, got + got4):
        np.testing.assert_array_equal(a, b)
    assert np.abs(ref[0]).max() > 0
    # the byte entry point: value = byte / 255, same results as the converted floats
    by = [np.round(a[:3] * 255.0).astype(np.uint8) for a in im]
    for a, b in zip(ref4, hard.computeFlowBatch(*by)):
        np.testing.assert_array_equal(a, b)
    import torch
    pin = [torch.from_numpy(a).pin_memory() for a in by]
    for a, b in zip(ref4, hard.computeFlowBatch(*[t.numpy() for t in pin])):
        np.testing.assert_array_equal(a, b)
    hard.set_option("host_subbatch_pixels", 16 << 20)


def test_host_path_graph_replay_identical(soft):
    """computeFlow replays a hipGraph from the third call of a shape on (eager, capture, replay): the results must
    not change by a bit, nor differ from a context with graphs switched off."""
    r = _rng(5)
    t = _triplet(r, 150, 200)
    soft.set_option("host_graph", 0)
    ref = soft.computeFlow(*t)
    soft.set_option("host_graph", 1)
    for _ in range(4):
        got = soft.computeFlow(*t)
        for a, b in zip(ref, got):
            np.testing.assert_array_equal(a, b)
    t2 = _triplet(r, 150, 200)                     # other data through the captured graph
    got2 = soft.computeFlow(*t2)
    soft.set_option("host_graph", 0)
    for a, b in zip(soft.computeFlow(*t2), got2):
        np.testing.assert_array_equal(a, b)
    soft.set_option("host_graph", 1)


def test_batch_equals_single(soft):
    """Kernel choice by map size (adaptive_kernels = 0): batching must not change a single bit.  The default (-1) picks the Winograd
    variant per launch for SINGLE-triplet calls (latency: the reference's own calling pattern, back2future.lua:73), so a triplet computed
    alone may differ from the same triplet inside a batch -- by fp32 rounding, far inside the 1e-3 contract; the masks may only differ
    where est[3] is within that distance of the threshold."""
    r = _rng(9)
    trip = [_triplet(r, 64, 128) for _ in range(3)]
    im = [np.stack([t[i] for t in trip]) for i in range(3)]
    with soft.options(adaptive_kernels=0):
        fb, fob, bob = soft.computeFlowBatch(*im)
        for i, t in enumerate(trip):
            f1, fo1, bo1 = soft.computeFlow(*t)
            np.testing.assert_array_equal(fb[i], f1)
            np.testing.assert_array_equal(fob[i], fo1)
            np.testing.assert_array_equal(bob[i], bo1)
    assert soft.get_option("adaptive_kernels") == -1
    fb, fob, bob = soft.computeFlowBatch(*im)
    for i, t in enumerate(trip):
        f1, fo1, bo1 = soft.computeFlow(*t)
        f2, _, _ = soft.computeFlow(*t)
        np.testing.assert_array_equal(f1, f2)           # deterministic per shape
        assert np.abs(fb[i] - f1).max() <= 2e-5
        assert (fob[i] != fo1).mean() <= 1e-3 and (bob[i] != bo1).mean() <= 1e-3


def test_graph_replay_matches_eager(soft):
    import torch
    r = _rng(21)
    B, H, Wd = 2, 64, 128
    x = torch.from_numpy(r.standard_normal((B, 9, H, Wd)).astype(np.float32)).cuda()
    outs = []
    for use_graph in (0, 1, 1, 1):        # eager; first sight (eager); capture + replay; replay
        soft.set_option("use_graph", use_graph)
        flow = torch.zeros(B, 2, H, Wd, device="cuda"); occ = torch.zeros(B, 2, H, Wd, device="cuda")
        torch.cuda.synchronize()                   # the fills run on torch's stream, the context on its own
        soft.forward_device(x.data_ptr(), B, H, Wd, flow.data_ptr(), occ.data_ptr())
        soft.synchronize()
        outs.append((flow.cpu().numpy(), occ.cpu().numpy()))
    soft.set_option("use_graph", 0)
    for f, o in outs[1:]:
        np.testing.assert_array_equal(f, outs[0][0])
        np.testing.assert_array_equal(o, outs[0][1])


def test_host_entry_point_refuses_device_memory(hard):
    import ctypes as C
    import torch
    from back2future_amd import _lib
    from back2future_amd._lib import B2FError
    x = torch.rand(3, 64, 64, device="cuda")
    flow = np.empty((2, 64, 64), np.float64); fo = np.empty((64, 64), np.uint8); bo = np.empty((64, 64), np.uint8)
    fp = C.cast(x.data_ptr(), _lib.c_float_p)
    rc = _lib.lib().b2f_compute_flow(hard._h, fp, fp, fp, 64, 64, flow.ctypes.data_as(C.POINTER(C.c_double)),
                                     fo.ctypes.data_as(C.POINTER(C.c_ubyte)), bo.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert rc != 0
    with pytest.raises(B2FError, match="device memory"):
        _lib.check(rc)


def test_errors_are_loud(hard):
    from back2future_amd._lib import B2FError
    with pytest.raises(B2FError, match="cannot open"):
        back2future.Model("Ours-Hard")            # models/RoamingImages_H.t7 is not in the tree (cwd = repo root)
    with pytest.raises(B2FError):
        back2future.Model("no-such-model")
    with pytest.raises(B2FError):
        hard.forward_device(1, 1, 100, 128)       # not a multiple of 64
    with pytest.raises(B2FError):
        hard.computeFlow(np.zeros((3, 32, 32), np.float32), np.zeros((3, 32, 32), np.float32),
                         np.zeros((3, 32, 32), np.float32))


@pytest.mark.parametrize("which", ["hard", "soft"])
def test_full_forward_table_vs_oracle(hard, soft, which):
    """b2f_forward (full model:forward table) against the oracle at 128 x 192, batch 2."""
    m = hard if which == "hard" else soft
    r = _rng(31)
    x = r.standard_normal((2, 9, 128, 192)).astype(np.float32)
    outs = m.forward(x)
    exp = O.pwc_forward(x, W.random_init(5, which == "soft", 2.0), which == "soft")
    assert len(outs) == len(exp) == m.n_outputs
    for i, (a, b) in enumerate(zip(outs, exp)):
        assert a.shape == b.shape
        assert np.abs(a - b).max() <= 1e-3, (i, float(np.abs(a - b).max()))


def test_init_from_t7_file_and_reference_names(tmp_path, hard):
    """back2future.init('Ours-Hard') resolves models/RoamingImages_H.t7 relative to the current
    directory (back2future.lua:100-113); the .t7 is read by the library itself."""
    import os
    from tests import t7_writer
    flat = W.random_init(5, False, 2.0)
    mdir = tmp_path / "models"
    mdir.mkdir()
    t7_writer.save(str(mdir / "RoamingImages_H.t7"), flat, False, dpt=True)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        m = back2future.Model("Ours-Hard")
    finally:
        os.chdir(cwd)
    assert not m.past_flow
    np.testing.assert_array_equal(m.get_weights(), flat)
    r = _rng(3)
    im = _triplet(r, 64, 128)
    f1, fo1, bo1 = m.computeFlow(*im)
    f2, fo2, bo2 = hard.computeFlow(*im)            # same weights through "random:hard:5:2.0"
    np.testing.assert_array_equal(f1, f2)
    np.testing.assert_array_equal(fo1, fo2)
    m.close()
    m2 = back2future.Model(str(mdir / "RoamingImages_H.t7"))
    np.testing.assert_array_equal(m2.get_weights(), flat)
    m2.close()


def test_reference_sample_triplet(soft):
    """BASELINE.json configs[0]: samples/frame_0009..0011.png (375 x 1242 -> net 320 x 1216, the
    host image.scale path at its real size).  The pretrained .t7 is not available, so the weights
    are the seeded random Soft set; bar 1e-3 on the rescaled flow."""
    import os
    from back2future_amd import flow_io
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
    ims = [flow_io.load_image(os.path.join(d, "frame_%04d.png" % i)) for i in (9, 10, 11)]
    assert ims[0].shape == (3, 375, 1242)
    flow, fo, bo = soft.computeFlow(*ims)
    eflow, efo, ebo, fnet, onet = O.compute_flow(ims[0], ims[1], ims[2], W.random_init(5, True, 2.0), True, want_net=True)
    assert fnet.shape == (2, 320, 1216)
    assert np.abs(flow - eflow).max() <= 1e-3
    near = O.image_scale_simple((np.abs(onet - 0.6666) < 1e-3).astype(np.uint8), 375, 1242).astype(bool)
    assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0


def test_c_harness_matches_python_mirror(tmp_path, hard):
    """examples/compute_flow.c (plain C over the C ABI, no Python / torch in the process) on a 150 x 200 triplet:
    the same bits as the ctypes mirror."""
    import subprocess
    from tests.test_cabi_cpu import _build_c_example
    exe = _build_c_example(tmp_path)
    r = _rng(8)
    H0, W0 = 150, 200
    ims = _triplet(r, H0, W0)
    np.concatenate(ims, 0).astype("<f4").tofile(str(tmp_path / "in.raw"))
    p = subprocess.run([exe, "random:hard:5:2.0", str(tmp_path / "in.raw"), str(H0), str(W0), str(tmp_path / "out.raw")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    raw = np.fromfile(str(tmp_path / "out.raw"), np.uint8)
    flow = raw[:16 * H0 * W0].view("<f8").reshape(2, H0, W0)
    occ = raw[16 * H0 * W0:].reshape(2, 1, H0, W0)
    eflow, efo, ebo = hard.computeFlow(*ims)
    np.testing.assert_array_equal(flow, eflow)
    np.testing.assert_array_equal(occ[0], efo)
    np.testing.assert_array_equal(occ[1], ebo)


def test_growing_shapes_match_a_fresh_context():
    """A long-lived context whose workspace arena, buffer sets and graph cache keep growing must give the bits a
    fresh context gives for every shape (regression: the arena used to be zeroed by an asynchronous null-stream
    memset that could land on top of the first kernels' output after it grew)."""
    r = _rng(77)
    old = back2future.Model("random:soft:4:2.0")
    try:
        for n, H0, W0 in [(1, 64, 64), (2, 100, 180), (3, 128, 256), (4, 200, 300), (5, 264, 374), (6, 320, 448), (2, 70, 90)]:
            ims = [r.random((n, 3, H0, W0), dtype=np.float32) for _ in range(3)]
            got = old.computeFlowBatch(*ims)
            fresh = back2future.Model("random:soft:4:2.0")
            try:
                exp = fresh.computeFlowBatch(*ims)
            finally:
                fresh.close()
            for a, b in zip(got, exp):
                np.testing.assert_array_equal(a, b)
    finally:
        old.close()


def test_context_stream_is_ordered_with_the_default_stream(hard):
    """Inputs produced on the default stream right before b2f_forward_device(stream = NULL), no synchronization in
    between: the context's stream is a blocking one, so it must see the finished inputs."""
    import torch
    B, H, Wd = 2, 128, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.rand((B, 9, H, Wd), generator=g, device="cuda")
    torch.cuda.synchronize()
    flow_ref = torch.empty(B, 2, H, Wd, device="cuda")
    hard.forward_device(base.data_ptr(), B, H, Wd, flow_ref.data_ptr(), unit_input=True)
    hard.synchronize()
    for _ in range(5):
        big = torch.rand((64, 1024, 1024), device="cuda")          # keeps the default stream busy for a while
        for _ in range(20):
            big = big * 1.0001 + 0.0
        x = base + (big[0, :1, :1] * 0.0)                            # depends on the whole chain
        flow = torch.empty(B, 2, H, Wd, device="cuda")
        hard.forward_device(x.data_ptr(), B, H, Wd, flow.data_ptr(), unit_input=True)
        hard.synchronize()
        assert torch.equal(flow, flow_ref)


def test_set_weights_hard_to_soft_on_a_warm_context():
    """b2f_set_weights on a context that has already captured hipGraphs for a shape: the Hard graphs (other packed
    buffer, 3-channel est[3], no second softmax) must not be replayed for the Soft model."""
    r = _rng(8)
    ims = _triplet(r, 128, 192)
    m = back2future.Model("random:hard:5:2.0")
    fresh = back2future.Model("random:soft:6:2.0")
    try:
        for _ in range(3):                               # eager, capture, replay
            h1 = m.computeFlow(*ims)
        m.set_weights(W.random_init(6, True, 2.0))
        assert m.past_flow
        for _ in range(3):
            got = m.computeFlow(*ims)
            exp = fresh.computeFlow(*ims)
            for a, b in zip(got, exp):
                np.testing.assert_array_equal(a, b)
        m.set_weights(W.random_init(5, False, 2.0))      # and back
        for _ in range(3):
            for a, b in zip(m.computeFlow(*ims), h1):
                np.testing.assert_array_equal(a, b)
    finally:
        m.close()
        fresh.close()


def test_broadcast_weights_device_path():
    """The multi-GPU weight path on one GPU: a world-size-1 RCCL group, context B initialised from ANOTHER seed, the
    flat buffer of A copied on the device into B's b2f_weights_device() buffer, RCCL broadcast in place on B's
    buffer (dist.broadcast_weights), b2f_commit_weights -- B must then compute A's bits."""
    import os
    import torch
    import torch.distributed as dist
    from back2future_amd import dist as D
    r = _rng(9)
    ims = _triplet(r, 128, 192)
    a = back2future.Model("random:hard:5:2.0")
    b = back2future.Model("random:hard:77:1.0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        exp = a.computeFlow(*ims)
        before = b.computeFlow(*ims)
        assert np.abs(before[0] - exp[0]).max() > 1e-3
        assert D.weights_checksum(a) != D.weights_checksum(b)
        pa, n = a.weights_device_ptr()
        pb, nb = b.weights_device_ptr()
        assert n == nb

        def wrap(ptr):
            class H(object):
                pass
            h = H()
            h.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
            return torch.as_tensor(h, device=torch.device("cuda", 0))
        wrap(pb).copy_(wrap(pa))                   # what a rank != src receives
        torch.cuda.synchronize()
        assert np.abs(b.computeFlow(*ims)[0] - before[0]).max() == 0      # packed copies still hold the old weights
        assert D.broadcast_weights(b, src=0) == n   # in-place RCCL broadcast + commit
        assert D.weights_checksum(a) == D.weights_checksum(b)
        for x, y in zip(b.computeFlow(*ims), exp):
            np.testing.assert_array_equal(x, y)
    finally:
        if created:
            dist.destroy_process_group()
        a.close()
        b.close()


def test_multi_gpu_two_replicas_on_one_gpu(monkeypatch):
    """The N > 1 code of the one-process multi-GPU entry points on the one-GPU test box: B2F_MULTI_ALLOW_DUPLICATE=1 (honoured only
    with the peer transport) lists GPU 0 twice -> two contexts, two worker threads, two uneven shards (5 = 3 + 2), replica 1 created
    from OTHER weights and brought in line by the peer broadcast; results bit-identical to one context, also where a shard holds a
    single triplet of a larger request (n = 3, 2); a failure on replica 1 is
    handed over from its worker thread to the caller with the GPU named; the pair keeps working afterwards (util.lua:27-48)."""
    import ctypes as C
    from back2future_amd import _lib
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    r = _rng(23)
    n, H0, W0 = 5, 100, 150
    ims = [r.random((n, 3, H0, W0), dtype=np.float32) for _ in range(3)]
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        assert mm.n_gpus == 2 and mm.devices == [0, 0] and mm.transport == "hipMemcpyPeer"
        sums = mm.weights_checksums()
        assert len(sums) == 2 and sums[0] == sums[1]
        assert back2future.shard_range(n, 0, 2) == (0, 3) and back2future.shard_range(n, 1, 2) == (3, 5)
        exp = ref.computeFlowBatch(*ims)
        for a, b in zip(mm.computeFlowBatch(*ims), exp):
            np.testing.assert_array_equal(a, b)
        by = [np.round(a * 255).astype(np.uint8) for a in ims]
        for a, b in zip(mm.computeFlowBatch(*by), ref.computeFlowBatch(*by)):
            np.testing.assert_array_equal(a, b)
        # one triplet: replica 1's shard is empty, only one worker thread runs
        for a, b in zip(mm.computeFlowBatch(*[x[:1] for x in ims]), [e[:1] for e in exp]):
            np.testing.assert_array_equal(a, b)
        # shards of one triplet (n = 3 -> 2 + 1, n = 2 -> 1 + 1) keep the kernel rule of the caller's n: at 256 x 512 a lone
        # triplet (per-launch rule) gets other bits than the same triplet in a batch (map-size rule)
        big = [r.random((3, 3, 256, 512), dtype=np.float32) for _ in range(3)]
        alone = ref.computeFlowBatch(*[x[2:] for x in big])
        assert not np.array_equal(alone[0][0], ref.computeFlowBatch(*big)[0][2])
        for ins in (big, [np.round(a * 255).astype(np.uint8) for a in big]):
            for k in (3, 2):
                for a, b in zip(mm.computeFlowBatch(*[x[:k] for x in ins]), ref.computeFlowBatch(*[x[:k] for x in ins])):
                    np.testing.assert_array_equal(a, b, err_msg="n = %d, %s" % (k, ins[0].dtype))
        # replica 1 fails once: the message crosses from its worker thread to the caller
        L = _lib.lib()
        _lib.check(L.b2f_set_option(C.c_void_p(L.b2f_multi_context(mm._h, 1)), b"debug_fail_next", 1))
        with pytest.raises(Exception, match="GPU 0: .*forced failure"):
            mm.computeFlowBatch(*ims)
        for a, b in zip(mm.computeFlowBatch(*ims), exp):
            np.testing.assert_array_equal(a, b)
    finally:
        mm.close()
        ref.close()
    # without the test switch a repeated device is refused
    monkeypatch.delenv("B2F_MULTI_ALLOW_DUPLICATE")
    with pytest.raises(Exception, match="listed twice|exceeds the visible devices"):
        back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])


def test_multi_gpu_entry_point_on_the_visible_gpus(monkeypatch):
    """b2f_init_multi / b2f_multi_compute_flow_batch on every visible GPU (one on the test box): the sharded batch must
    equal the single-context results bit for bit, and every replica must hold replica 0's weights.  With one GPU the
    weight broadcast is still driven through RCCL (communicator of one rank, in-place ncclBroadcast)."""
    import torch
    if torch.cuda.device_count() == 1:
        monkeypatch.setenv("B2F_MULTI_TRANSPORT", "selftest")
    r = _rng(21)
    n, H0, W0 = 5, 100, 150
    ims = [r.random((n, 3, H0, W0), dtype=np.float32) for _ in range(3)]
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=0)
    ref = back2future.Model("random:soft:5:2.0")
    try:
        assert mm.n_gpus == torch.cuda.device_count() >= 1
        assert len(set(mm.weights_checksums())) == 1
        assert mm.transport in ("RCCL broadcast", "hipMemcpyPeer"), mm.transport
        got = mm.computeFlowBatch(*ims)
        exp = ref.computeFlowBatch(*ims)
        for a, b in zip(got, exp):
            np.testing.assert_array_equal(a, b)
        by = [np.round(a * 255).astype(np.uint8) for a in ims]
        for a, b in zip(mm.computeFlowBatch(*by), ref.computeFlowBatch(*by)):
            np.testing.assert_array_equal(a, b)
        with pytest.raises(Exception):
            back2future.MultiModel("random:hard", n_gpus=mm.n_gpus + 7)
    finally:
        mm.close()
        ref.close()


@pytest.mark.parametrize("C,h,w,scale", [(3, 9, 11, 1.5), (40, 7, 13, 3.0), (128, 6, 5, 0.4), (32, 1, 4, 2.0)])
def test_warp_bhwd_backward(hard, C, h, w, scale):
    """BilinearSamplerBHWD:updateGradInput (BilinearSamplerBHWD.cu:161-307) vs the oracle: the grid gradient reduces in
    the reference's own order (bit-exact), the image gradient is an atomic scatter (order-free tolerance)."""
    r = _rng(C * h + w)
    img = r.standard_normal((2, h, w, C), dtype=np.float32)
    grid = (r.standard_normal((2, h, w, 2)) * scale).astype(np.float32)       # incl. points clamped at the border
    go = r.standard_normal((2, h, w, C), dtype=np.float32)
    gi, gg = ops.warp_bhwd_backward(hard, img, grid, go)
    ei, eg = O.warp_bhwd_backward(img, grid, go)
    np.testing.assert_array_equal(gg, eg)
    np.testing.assert_allclose(gi, ei, rtol=1e-5, atol=1e-5)
    gi2, gg2 = ops.warp_bhwd_backward(hard, img, grid, go, only_grid=True)
    assert gi2 is None
    np.testing.assert_array_equal(gg2, eg)


@pytest.mark.parametrize("C,h,w,win,fwd", [(6, 10, 12, 9, True), (6, 10, 12, 9, False), (32, 7, 5, 5, True), (8, 3, 4, 3, False), (16, 1, 9, 9, True)])
def test_costvol_backward(hard, C, h, w, win, fwd):
    """CostVolMulti:updateGradInput (CostVolMulti.lua:111-181): same sequence of fp32 operations as the Lua loops."""
    r = _rng(C + h * w + win)
    ref = r.standard_normal((2, C, h, w), dtype=np.float32)
    frm = r.standard_normal((2, C, h, w), dtype=np.float32)
    go = r.standard_normal((2, win * win, h, w), dtype=np.float32)
    gr, gf = ops.costvol_backward(hard, ref, frm, go, win, fwd)
    er, ef = O.costvol_backward(ref, frm, go, win, fwd)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gf, ef)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
@pytest.mark.parametrize("ci,co,h,w,blocks,mode", [(128, 128, 40, 70, 3, 1), (200, 128, 33, 65, 5, 2), (32, 64, 17, 100, 2, 1), (104, 192, 48, 33, 7, 1),
                                                   (64, 100, 70, 31, 64, 2), (96, 96, 16, 32, 2, 1), (8, 64, 1, 1, 1, 2), (40, 36, 5, 3, 1, 2)])
def test_conv3x3_one_dimensional_winograd_on_the_bf16_pipe(hard, scale, ci, co, h, w, blocks, mode):
    """Option wino1d (b2f_w1b.hip): the stride-1 layers as a one-dimensional Winograd F(4,3) along x on the bf16 matrix pipe with every
    fp32 operand split exactly into three bf16 terms (six of nine term products), in loader / consumer persistent blocks.  1 = the
    n-blocks with more than 32 real outputs (a last block of <= 32 stays on the F(4x4) kernel), 2 = every n-block.  Against the oracle
    at a bar three times tighter than F(4x4)'s, against an fp64 convolution no worse than the fp32 F(4x4) kernel, and the bits must not
    depend on how many persistent blocks walk the tiles."""
    import torch
    r = _rng(ci * 13 + co + blocks)
    x = (r.standard_normal((3, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = (r.standard_normal(co, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(wino4_persistent=blocks, wino1d=0):
        f32 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino4_persistent=blocks, wino1d=mode):
        got = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino4_persistent=1, wino1d=mode):
        got1 = ops.conv3x3(hard, x, wt, b, 1, True)
    assert not np.array_equal(got, f32)                      # the other kernel really ran
    np.testing.assert_allclose(got, O.conv3x3(x, wt, b, 1, True), rtol=1e-4, atol=5e-5 * scale)
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert es.max() <= max(ef.max(), 1e-5 * scale) and es.mean() <= max(ef.mean(), 1e-6 * scale)
    assert np.array_equal(got, got1)


def test_compute_flow_with_the_one_dimensional_winograd_kernel(hard):
    """The whole graph with the F(4x4)-class layers on b2f_w1b.hip (wino1d = 1, 2; wino4_min_pixels = 0 sends every eligible layer
    there at this size): the end-to-end bar of the default path; switching the option repacks the weights and back."""
    r = _rng(15)
    H, Wd = 128, 256
    ims = _triplet(r, H, Wd)
    eflow, efo, ebo, fnet, onet = O.compute_flow(*ims, W.random_init(5, False, 2.0), False, want_net=True)
    with hard.options(wino4_min_pixels=0, adaptive_kernels=0, host_graph=0):
        base, _, _ = hard.computeFlow(*ims)
        for mode in (1, 2):
            with hard.options(wino1d=mode):
                flow, fo, bo = hard.computeFlow(*ims)
            d = np.abs(flow - eflow)
            assert np.abs(eflow).max() > 0.02 and d.max() <= 1e-3, (mode, d.max())
            assert not np.array_equal(flow, base) and np.abs(flow - base).max() < 1e-5     # another kernel, the same function
            near = np.abs(onet - 0.6666) < 1e-3
            assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0
        again, _, _ = hard.computeFlow(*ims)
    assert np.array_equal(again, base)


def test_kernel_mix_options_drop_the_captured_graphs(hard):
    """bf16_direct / bf16_conv change which kernels a forward pass launches: a hipGraph captured before the change must not be replayed
    after it (the options synchronise and drop the captured graphs like every other kernel-mix option)."""
    r = _rng(31)
    ims = _triplet(r, 128, 256)
    with hard.options(host_graph=1):
        a, _, _ = hard.computeFlow(*ims)
        a2, _, _ = hard.computeFlow(*ims)                   # replayed
        with hard.options(bf16_direct=0, bf16_conv=0):
            b, _, _ = hard.computeFlow(*ims)
            b2, _, _ = hard.computeFlow(*ims)
        c, _, _ = hard.computeFlow(*ims)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(a, c)
    assert not np.array_equal(a, b) and np.abs(a - b).max() < 2e-5


def test_direct_kernels_everywhere_end_to_end():
    """B2F_WINO=0 (the parity switch of INTEGRATION.md): every layer on the direct fp32-MFMA implicit-GEMM kernel -- the layers of the
    head are then packed for that kernel, so the fused head kernel (which reads the c16 / c16s2 packings) must not run."""
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import numpy as np\n"
        "from back2future_amd import back2future, weights as W\n"
        "from oracle import oracle as O\n"
        "r = np.random.default_rng(5)\n"
        "base = r.random((3, 136, 264)).astype(np.float32)\n"
        "ims = [base[:, 4:132, 4:260], base[:, 3:131, 2:258], base[:, 2:130, 0:256]]\n"
        "m = back2future.Model('random:hard:5:2.0')\n"
        "assert m.get_option('bf16_direct') == 0 and m.get_option('bf16_conv') == 0\n"
        "flow, fo, bo = m.computeFlow(*ims)\n"
        "eflow, efo, ebo = O.compute_flow(*ims, W.random_init(5, False, 2.0), False)\n"
        "d = float(np.abs(flow - eflow).max())\n"
        "assert np.abs(eflow).max() > 0.02 and d <= 1e-3, d\n"
        "print('ok', d)\n")
    env = dict(os.environ, B2F_WINO="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_environment_cannot_name_a_kernel_that_is_not_in_the_build():
    """B2F_<OPTION> seeds an option at b2f_init with the rule b2f_set_option enforces: an experiment kernel that the product build does not
    hold (cost-volume variants 2/4/6/8, bf16_direct = 1) is not accepted under its name -- get_option reports what runs."""
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "from back2future_amd import back2future\n"
        "m = back2future.Model('random:hard:5:2.0')\n"
        "exp = m.get_option('experiments')\n"
        "cv, bd = m.get_option('corr_variant'), m.get_option('bf16_direct')\n"
        "assert (cv, bd) == ((4, 1) if exp else (-1, 2)), (exp, cv, bd)\n"
        "assert m.get_option('wino6') == 0\n"
        "print('ok')\n")
    env = dict(os.environ, B2F_CORR_VARIANT="4", B2F_BF16_DIRECT="1", B2F_WINO6="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("B,ci,co,h,w,scale,blocks", [(1, 64, 96, 16, 64, 1.0, 1), (2, 32, 64, 37, 71, 1.0, 3), (1, 64, 96, 33, 50, 300.0, 1), (3, 96, 128, 9, 130, 1e-3, 2),
                                                      (1, 128, 192, 32, 60, 1.0, 1), (2, 40, 64, 20, 20, 1.0, 1), (1, 64, 100, 31, 33, 1.0, 7), (1, 24, 32, 40, 66, 1.0, 1),
                                                      (1, 8, 256, 2, 2, 1.0, 1), (4, 16, 36, 1, 1, 1.0, 1), (3, 72, 160, 64, 48, 1.0, 5), (1, 64, 96, 8, 16, 1.0, 2)])
def test_stride2_loader_consumer_kernel(hard, B, ci, co, h, w, scale, blocks):
    """b2f_s2b.hip (option s2_loader; 2 = every stride-2 layer, the default 1 = those of at least 64 input channels): the stride-2 convs of
    pwc.lua:60 on the bf16 pipe with split fp32 operands in loader / consumer persistent blocks that compute all outputs of a tile.
    Against the oracle at the direct kernels' bar, against an fp64 convolution no worse than the fp32-MFMA kernel, the same bits for
    every number of persistent blocks -- and the same bits as conv3x3_bf6 (the same products summed in the same order)."""
    import torch
    r = _rng(ci * 7 + co + h)
    x = (r.standard_normal((B, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = (r.standard_normal(co, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1, stride=2)
    exp = torch.where(y > 0, y, 0.2 * y).numpy()
    with hard.options(bf16_conv=0):
        f32 = ops.conv3x3(hard, x, wt, b, 2, True)
    with hard.options(bf16_conv=1, s2_loader=0):
        bf6 = ops.conv3x3(hard, x, wt, b, 2, True)
    with hard.options(bf16_conv=1, s2_loader=2, wino4_persistent=blocks):
        got = ops.conv3x3(hard, x, wt, b, 2, True)
    with hard.options(bf16_conv=1, s2_loader=2, wino4_persistent=1):
        got1 = ops.conv3x3(hard, x, wt, b, 2, True)                  # small launches: one output tile per block (s2_tile_groups, the default)
    with hard.options(bf16_conv=1, s2_loader=2, wino4_persistent=1, s2_tile_groups=0):
        got0 = ops.conv3x3(hard, x, wt, b, 2, True)                  # always all outputs of a tile per block
    assert np.array_equal(got1, got0)
    np.testing.assert_allclose(got, O.conv3x3(x, wt, b, 2, True), rtol=2e-5, atol=2e-5 * scale)
    es, ef = np.abs(got - exp), np.abs(f32 - exp)
    assert es.max() <= 1e-4 * scale and es.max() <= 1.5 * ef.max() + 1e-6 * scale
    assert np.array_equal(got, got1)
    if (co & 3) == 0:
        assert np.array_equal(got, bf6)


@pytest.mark.parametrize("B,ci,co,h,w", [(1, 64, 32, 16, 30), (1, 200, 128, 16, 30), (1, 128, 96, 32, 60), (3, 96, 64, 9, 17), (1, 40, 32, 8, 16), (2, 72, 160, 17, 33),
                                         (1, 562, 128, 16, 30), (1, 8, 32, 1, 1), (1, 136, 64, 64, 120)])
def test_conv3x3_wino_eight_wave_form_bit_identical(hard, B, ci, co, h, w):
    """conv3x3_wino8 (option wino8, default on): the one-N-tile F(2x2) launches of at most one block per CU -- a single triplet's coarse
    levels -- on 512-thread blocks whose waves multiply one xi pair each.  Same operations per output in the same order: the bits of the
    four-wave kernel, split into 32-output blocks or not, and the oracle's values at the F(2x2) bar."""
    r = _rng(ci + 3 * co + h)
    x = r.standard_normal((B, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    big = 1 << 30
    with hard.options(wino8=0, wino4_min_pixels=big, wino_split_pixels=big):
        a4 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino8=1, wino4_min_pixels=big, wino_split_pixels=big):
        a8 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino8=1, wino4_min_pixels=big, wino_split_pixels=0):
        a8n = ops.conv3x3(hard, x, wt, b, 1, True)
    np.testing.assert_array_equal(a4, a8)
    np.testing.assert_array_equal(a4, a8n)
    np.testing.assert_allclose(a8, O.conv3x3(x, wt, b, 1, True), rtol=2e-5, atol=1e-4)      # F(2x2) rounding on up to 562 input channels


@pytest.mark.parametrize("ci,co,h,w,blocks", [(128, 128, 40, 70, 3), (200, 128, 33, 65, 5), (32, 64, 17, 100, 2), (104, 192, 48, 33, 7), (64, 100, 70, 31, 64),
                                              (40, 160, 16, 32, 2), (32, 32, 49, 35, 5), (128, 96, 36, 83, 17), (64, 32, 20, 70, 3), (232, 128, 12, 48, 1),
                                              (264, 128, 6, 6, 1), (72, 36, 25, 49, 4)])
def test_conv3x3_wino6(hard, ci, co, h, w, blocks):
    """Winograd F(6x6,3x3) (csrc/b2f_wino6.hip, option wino6 -- the default kernel of the wide stride-1 layers on maps of at least
    wino6_min_pixels pixels), forced at test sizes: blocks of 64 outputs and the 32-output block of layers whose outputs are <= 32 mod 64,
    odd and even chunk counts, ragged edges, one to many items per persistent block.  Against the oracle at the bars of the F(4x4)
    kernel (tools/wino6_numerics.py: its fp32 rounding is 1.3 - 2.8 x F(4x4)'s and inside them), against an fp64 convolution within
    3 x the F(4x4) kernel's own error, and bit for bit against itself with another number of blocks (batching must not change a bit)."""
    import torch
    r = _rng(ci * 13 + co + blocks)
    x = r.standard_normal((3, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.standard_normal(co, dtype=np.float32)
    with hard.options(wino6=0):
        f4 = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino6=1, wino6_min_pixels=0):
        with hard.options(wino4_persistent=blocks):          # values > 1: exactly that many persistent blocks
            got = ops.conv3x3(hard, x, wt, b, 1, True)
        full = ops.conv3x3(hard, x, wt, b, 1, True)
    exp = O.conv3x3(x, wt, b, 1, True)
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1.5e-4)
    assert np.abs(got - exp).mean() < 5e-6
    assert np.array_equal(got, full)
    assert not np.array_equal(got, f4)                       # the other kernel really ran
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    e64 = torch.where(y > 0, y, 0.2 * y).numpy()
    assert np.abs(got - e64).max() <= 3.0 * np.abs(f4 - e64).max() + 1e-5


@pytest.mark.parametrize("scale", [1e-3, 30.0, 1e3])
@pytest.mark.parametrize("ci,co,h,w", [(128, 128, 33, 65), (200, 96, 40, 70)])
def test_conv3x3_wino6_activation_scale(hard, scale, ci, co, h, w):
    """The F(6x6) transforms (coefficients up to 32 in A^T, 21/4 in B^T) amplify fp32 rounding RELATIVE to the activations: the error bars must
    hold in proportion at any activation scale (the bias rides in the accumulators: scaled with the activations here, and not at all below)."""
    r = _rng(int(ci + co + scale) + 1)
    x = (r.standard_normal((2, ci, h, w), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    for bscale in (scale, 1.0):
        b = (r.standard_normal(co, dtype=np.float32) * np.float32(bscale)).astype(np.float32)
        with hard.options(wino6=1, wino6_min_pixels=0):
            got = ops.conv3x3(hard, x, wt, b, 1, False)
        exp = O.conv3x3(x, wt, b, 1, False)
        np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1.5e-4 * max(scale, bscale))
        assert np.abs(got - exp).mean() < 5e-6 * max(scale, bscale)


def test_compute_flow_with_the_f6x6_kernel(hard):
    """The whole graph with every F(4x4)-class layer on the F(6x6) kernel (wino6_min_pixels = 0 and wino4_min_pixels = 0 send every eligible layer
    there at this size): the end-to-end bar of the contract, and 1e-5 of the F(4x4) path on the flow (another kernel, the same function)."""
    r = _rng(16)
    H, Wd = 128, 256
    ims = _triplet(r, H, Wd)
    eflow, efo, ebo, fnet, onet = O.compute_flow(*ims, W.random_init(5, False, 2.0), False, want_net=True)
    with hard.options(wino4_min_pixels=0, adaptive_kernels=0, host_graph=0):
        with hard.options(wino6=0):
            base, _, _ = hard.computeFlow(*ims)
        with hard.options(wino6=1, wino6_min_pixels=0):
            flow, fo, bo = hard.computeFlow(*ims)
        with hard.options(wino6=0):
            again, _, _ = hard.computeFlow(*ims)
    d = np.abs(flow - eflow)
    assert np.abs(eflow).max() > 0.02 and d.max() <= 1e-3, d.max()
    assert not np.array_equal(flow, base) and np.abs(flow - base).max() < 1e-5
    assert np.array_equal(again, base)
    near = np.abs(onet - 0.6666) < 1e-3
    assert ((fo != efo) & ~near[1:2]).sum() == 0 and ((bo != ebo) & ~near[0:1]).sum() == 0


def test_multi_gpu_eight_replicas_partition_of_config4(monkeypatch):
    """BASELINE.json configs[4]'s partition on the one-GPU box: EIGHT replicas (B2F_MULTI_ALLOW_DUPLICATE lists GPU 0 eight times: eight contexts,
    eight worker threads, the peer broadcast from replica 0), n = 128 byte triplets -> 16 per replica, and an uneven n = 100 -> 13, 13, 13, 13,
    12, 12, 12, 12 (the contiguous dim-1 split of nn.DataParallelTable, util.lua:27-48), through b2f_multi_compute_flow_batch_u8 straight into
    the caller's buffers: bit-identical to one context.  (Small frames: the partition is what is tested, not the throughput.)"""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    r = _rng(29)
    H0, W0 = 64, 128
    by = [r.integers(0, 256, (128, 3, H0, W0), dtype=np.uint8) for _ in range(3)]
    mm = back2future.MultiModel("random:hard:3:2.0", n_gpus=8, devices=[0] * 8)
    ref = back2future.Model("random:hard:3:2.0")
    try:
        assert mm.n_gpus == 8 and len(set(mm.weights_checksums())) == 1
        assert [back2future.shard_range(128, i, 8) for i in range(8)] == [(16 * i, 16 * i + 16) for i in range(8)]
        sizes = [back2future.shard_range(100, i, 8)[1] - back2future.shard_range(100, i, 8)[0] for i in range(8)]
        assert sizes == [13, 13, 13, 13, 12, 12, 12, 12]
        exp = ref.computeFlowBatch(*by)
        for a, b in zip(mm.computeFlowBatch(*by), exp):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(mm.computeFlowBatch(*[x[:100] for x in by]), [e[:100] for e in exp]):
            np.testing.assert_array_equal(a, b)
        assert float(np.abs(exp[0]).max()) > 0.01
    finally:
        mm.close()
        ref.close()
