"""GPU: the small kernels of a forward pass -- csrc/b2f_glue.hip, csrc/b2f_seq.hip, the node kernels of csrc/b2f_graph.hip -- each through
its own op entry on the forward's strides, against the float64 restatements of tests/glue_float64.py.

Per kernel, shape and input family: |got - reference| <= n 2^-24 S elementwise with n counted at the source lines of
glue_float64.ROUNDINGS (0 where S = 0; copies and scale by 2.0: equality on bits); the worst err / (2^-24 S) is at most 2 x the float32
emulation's on the same family (tests/golden/glue_float64_ratios.json, held to a fresh computation by tests/test_glue_float64_cpu.py; the
factor is the conv test's, not a measurement of these kernels); `integers` bit for bit where the CPU file shows the case exact.  Records carry
NaN in every slot the kernel does not own and every device buffer starts as NaN between guards, so a read of a foreign slot or an element
left out shows as NaN.  The softmax is bounded by (2 E + 3) 2^-24 p + 2^-126 with E = twice the error of the device's expf measured here
against float64 exp on the tests' own arguments (ROCm's installed documentation states no accuracy for expf).
Run with -s for the table (profiles/r21_glue_float64.txt is that printout)."""
import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import conv_float64 as CF
from tests import cv_float64 as CV
from tests import glue_float64 as G

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
TABLE = {}          # (kernel, family) -> [worst err / (u S), cases, the emulation's, n]
NAN_WORD = 0x7fc0a5a5          # what an op entry's device buffer holds until a kernel writes it (csrc/b2f_ctx.h: kGuardWord)

# every __global__ kernel of the three files -> the test here (or elsewhere) that runs it through an op entry;
# tests/test_glue_float64_cpu.py holds this map to the sources
KERNEL_CASES = {
    "pack_input_kernel": "test_pack_input", "upsample_flow2x_kernel": "test_upsample", "softmax_nearest4_kernel": "test_softmax_nearest4",
    "warp_image_planar_kernel": "test_image_warps", "warp_input_planar_kernel": "test_image_warps", "warp_input_seq_kernel": "test_image_warps",
    "avgpool2_kernel": "test_avgpool2", "nhwc_to_planar_kernel": "test_layout_kernels", "cp8_to_planar_kernel": "test_layout_kernels",
    "planar_to_nhwc_kernel": "test_layout_kernels", "conv_first_seq_kernel": "test_conv_first_seq", "expf_kernel": "test_softmax_nearest4",
    "put_channels_kernel": "test_put_channels", "costvol_cp8_kernel": "test_costvol_cp8", "warp_cp8_kernel": "test_warp_cp8",
    "add_flow_kernel": "test_add_flow_and_scale", "scale_kernel": "test_add_flow_and_scale", "softmax_nearest_kernel": "test_softmax_nearest4",
    # held elsewhere
    "warp_nhwc_kernel": "tests/test_gpu_reference_sampler.py (ops.warp_bhwd)", "conv_first_kernel": "tests/test_gpu_conv_float64.py",
    "conv_narrow2_kernel": "tests/test_gpu_conv_float64.py", "fill_kernel": "excepted: a memset",
}


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n%-18s %-9s %12s %12s %8s %6s" % ("kernel", "family", "worst/(uS)", "emulation", "bound n", "cases"))
    for (kernel, family), (worst, cases, emu, n) in sorted(TABLE.items()):
        print("%-18s %-9s %12.3f %12.3f %8.1f %6d" % (kernel, family, worst, emu, n, cases))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(kernel, family, got, val, S, n, what, row=None):
    """the bound and the 2 x emulation bar on one result: the list of failures"""
    r = G.measure(got, val, S)
    emu = G.recorded(row or kernel, family)
    t = TABLE.setdefault((row or kernel, family), [0.0, 0, emu, n])
    t[0], t[1], t[3] = max(t[0], r), t[1] + 1, max(t[3], n)
    print("%-60s %-9s err / (u S) = %8.3f (n = %3d, emulation %7.3f)" % (what, family, r, n, emu))
    fails = []
    if not r <= n:
        fails.append("%s %s: error %.3f u S exceeds the bound n = %d" % (what, family, r, n))
    if not r <= G.MARGIN * emu:
        fails.append("%s %s: err / (u S) = %.3f, more than %g x the emulation's %.3f" % (what, family, r, G.MARGIN, emu))
    return fails


# ---- upsampling ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", G.UPSAMPLE_SHAPES, ids=lambda v: str(v))
def test_upsample(hard, h, w):
    """launch_upsample_flow2x on 8-float records (every level of the forward) and on packed pairs (the second step, the executor),
    launch_upsample_flow2x_planar on packed pairs: the three give the same bits; b2f_glue.hip:96-97"""
    fails = []
    for B in G.UPSAMPLE_BATCHES:
        for family in G.FAMILIES:
            x, val, S = G.upsample_case(family, B, h, w)
            y8 = ops.upsample_flow2x_records(hard, G.records(x, 8))
            y2 = ops.upsample_flow2x_records(hard, G.records(x, 2))
            yp = ops.upsample_flow2x_records(hard, G.records(x, 2), planar=True)
            what = "upsample %dx%d B %d" % (h, w, B)
            if not _same(y8, y2):
                fails.append("%s %s: ps = 8 and ps = 2 differ in %d outputs" % (what, family, int((_bits(y8) != _bits(y2)).sum())))
            if not _same(np.moveaxis(y2, 3, 1), yp):
                fails.append("%s %s: the NHWC and planar forms differ" % (what, family))
            if not _same(ops.upsample_flow2x(hard, x), yp):
                fails.append("%s %s: b2f_op_upsample_flow2x differs from the planar form" % (what, family))
            fails += _check("upsample", family, yp, val, S, G.n_of("upsample"), what)
            if family == "integers" and (h, w) in G.UPSAMPLE_EXACT and not _same(yp, val.astype(f32)):
                fails.append("%s integers: not the exact result" % what)
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


def test_upsample_refuses_a_map_past_the_grid(hard):
    h, w = G.UPSAMPLE_REFUSED
    x = np.zeros((1, h, w, 2), f32)
    for planar in (False, True):
        with pytest.raises(_lib.B2FError, match="launch_upsample_flow2x"):
            ops.upsample_flow2x_records(hard, x, planar=planar)
    with pytest.raises(_lib.B2FError, match="launch_upsample_flow2x"):
        ops.upsample_flow2x_records(hard, np.zeros((1, h, w, 8), f32))
    with pytest.raises(_lib.B2FError, match="bad shape"):
        ops.upsample_flow2x_records(hard, np.zeros((1, 2, 2, 3), f32))
    assert ops.upsample_flow2x_records(hard, np.ones((1, 1, 1, 2), f32)).tolist() == [[[[1.0, 1.0]] * 2] * 2]


# ---- softmax -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def expf_error(hard):
    """E of the device's expf on every z - m of the softmax cases, in units of 2^-24 exp"""
    args = np.concatenate([G.softmax_args(G.softmax_logits(B, h, w)[0]).reshape(-1) for (h, w) in G.SOFTMAX_SHAPES for B in G.SOFTMAX_BATCHES])
    got = ops.expf(hard, args)
    E = G.exp_error(args, got)
    sub = np.exp(args.astype(f64)) < G.TINY
    print("\nexpf on %d arguments of the softmax cases: worst |expf - exp| / (2^-24 exp) = %.4f where exp >= 2^-126; below (%d arguments) the "
          "worst |expf - exp| = %.3g" % (args.size, E, int(sub.sum()), float(np.abs(got.astype(f64) - np.exp(args.astype(f64)))[sub].max()) if sub.any() else 0.0))
    TABLE[("expf", "logits")] = [E, args.size, 0.0, 0]
    assert (got[args == 0] == 1).all()
    return E


@pytest.mark.parametrize("h,w", G.SOFTMAX_SHAPES, ids=lambda v: str(v))
def test_softmax_nearest4(hard, expf_error, h, w):
    """launch_softmax_nearest4_planar on 8-float records (b2f_glue.hip:166-174) and the executor's softmax_nearest (b2f_graph.hip:144-150)"""
    n = G.softmax_n(expf_error)
    fails = []
    for B in G.SOFTMAX_BATCHES:
        z, cls = G.softmax_logits(B, h, w)
        p64 = G.softmax(z, "64")
        out = ops.softmax_nearest4(hard, G.records(z, 8))
        what = "softmax_nearest4 %dx%d B %d" % (h, w, B)
        p = out[:, :, ::4, ::4]
        if not _same(out, G.nearest(p, 4)):
            fails.append(what + ": a 4 x 4 block is not one value")
        if not ((p[:, 0][cls >= 6] == 0.5).all() and (p[:, 1][cls >= 6] == 0.5).all()):
            fails.append(what + ": equal logits do not give exactly 0.5 and 0.5")
        if not (np.abs(p[:, 0].astype(f64) + p[:, 1].astype(f64) - 1.0) <= 2 * 2.0 ** -23).all():
            fails.append(what + ": p0 + p1 is more than 2 ulp from 1")
        r = G.softmax_ratio(p, p64)
        emu = G.recorded("softmax", "logits")
        t = TABLE.setdefault(("softmax", "logits"), [0.0, 0, emu, n])
        t[0], t[1] = max(t[0], r), t[1] + 1
        print("%-60s err / (u p + 2^-126) = %.3f (bound 2 E + 3 = %.2f, emulation %.3f)" % (what, r, n, emu))
        if not r <= n:
            fails.append("%s: error %.3f u p exceeds 2 E + 3 = %.3f" % (what, r, n))
        if not r <= G.MARGIN * emu:
            fails.append("%s: err / (u p) = %.3f, more than %g x the emulation's %.3f" % (what, r, G.MARGIN, emu))
        for f in (1, 2, 4, 8):
            g = ops.graph_softmax_nearest(hard, G.records(z, 8), f)
            if not _same(g, G.nearest(p, f)):
                fails.append("%s: the executor's softmax_nearest with f = %d does not give softmax_nearest4's bits" % (what, f))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


def test_softmax_refuses_a_map_past_the_grid(hard):
    h, w = G.SOFTMAX_REFUSED
    with pytest.raises(_lib.B2FError, match="launch_softmax_nearest4_planar"):
        ops.softmax_nearest4(hard, np.zeros((1, h, w, 8), f32))
    assert (ops.softmax_nearest4(hard, np.zeros((1, 1, 1, 8), f32)) == 0.5).all()


# ---- pooling, packing -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", G.AVGPOOL_SHAPES, ids=lambda v: str(v))
def test_avgpool2(hard, H, W):
    """launch_avgpool2_nhwc with C = 8, the image records; b2f_glue.hip:496-499"""
    fails = []
    for nimg in G.AVGPOOL_NIMG:
        for family in G.FAMILIES:
            x = G.avgpool_input(family, nimg, H, W)
            got = ops.avgpool2(hard, x)
            val = G.avgpool(x, "64")
            what = "avgpool2 %dx%d n %d" % (H, W, nimg)
            fails += _check("avgpool", family, got, val, G.avgpool(x, "abs"), G.n_of("avgpool"), what)
            if family == "integers" and not _same(got, val.astype(f32)):
                fails.append(what + " integers: not the exact result")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H,W", G.PACK_SHAPES, ids=lambda v: str(v))
def test_pack_input(hard, H, W):
    """launch_pack_input: copies without ColorNormalize (equality), two roundings with it (b2f_internal.h:187-191); channels 3..7 exactly +0"""
    fails = []
    for family in G.FAMILIES:
        x9 = G.image_frames(family, 2, H, W)
        for norm in (False, True):
            got = ops.pack_input(hard, x9, norm)
            what = "pack_input %dx%d%s" % (H, W, " normalized" if norm else "")
            if _bits(got[..., 3:]).any():
                fails.append("%s %s: channels 3..7 are not +0" % (what, family))
            if not norm:
                if not _same(got, G.pack(x9, False, "32")):
                    fails.append("%s %s: not a copy" % (what, family))
            else:
                val = G.pack(x9, True, "64")
                fails += _check("pack-norm", family, got, val, np.abs(val), G.n_of("pack-norm"), what)
    assert not fails, "\n".join(fails)


# ---- image warps ----------------------------------------------------------------------------------------------------------------------------------

def _copies(img, flow, cls, k):
    """(mask B x H x W, expected B x C x H x W) of the pixels whose two flow components are zero, a whole-pixel shift or an exact edge target:
    the clamped copy of the input"""
    B, C, H, W = img.shape
    ok = np.isin(cls[:, 0], (0, 1, 4)) & np.isin(cls[:, 1], (0, 1, 4))
    tx = np.clip(np.arange(W)[None, None, :] + np.rint(flow[:, 0].astype(f64) * k).astype(np.int64), 0, W - 1)
    ty = np.clip(np.arange(H)[None, :, None] + np.rint(flow[:, 1].astype(f64) * k).astype(np.int64), 0, H - 1)
    want = np.stack([img[b][:, ty[b], tx[b]] for b in range(B)])
    return ok, want


@pytest.mark.parametrize("B", G.WARP_BATCHES)
@pytest.mark.parametrize("H,W", G.WARP_SHAPES, ids=lambda v: str(v))
def test_image_warps(hard, H, W, B):
    """launch_warp_image_planar on launch_pack_input's frames, launch_warp_input_planar and launch_warp_input_seq on the same frame: the same
    bits on finite images, normalized or not; the bound (b2f_glue.hip:207-210,458-467, b2f_seq.hip:122-131); copies bit for bit; bytes give
    the bits of their float32 values k / 255"""
    fails = []
    for k in G.WARP_K:
        for family in G.FAMILIES:
            x9 = G.image_frames(family, B, H, W)
            flow, cls = G.warp_flow(family, B, H, W, k)
            img = np.ascontiguousarray(x9[:, :3])
            for norm in (False, True):
                a = ops.warp_image(hard, "image", ops.pack_input(hard, x9, norm)[0], flow, k)
                b = ops.warp_image(hard, "input", x9, flow, k, normalized=not norm, frame=0)
                c = ops.warp_image(hard, "seq", img, flow, k, normalized=not norm)
                what = "image warps %dx%d B %d k %g%s" % (H, W, B, k, " normalized" if norm else "")
                if not (_same(a, b) and _same(a, c)):
                    fails.append("%s %s: the three kernels differ (image / input: %d, image / seq: %d outputs)" % (
                        what, family, int((_bits(a) != _bits(b)).sum()), int((_bits(a) != _bits(c)).sum())))
                v64 = G.normalize(img, "64") if norm else img
                kern = "warp-norm" if norm else "warp"
                fails += _check(kern, family, a, G.warp(v64, flow, k, "64"), G.warp(v64, flow, k, "abs"), G.n_of(kern), what)
                if not norm and family == "integers" and not _same(a, G.warp(img, flow, k, "64").astype(f32)):
                    fails.append(what + " integers: not the exact result")
                if not norm and cls is not None:
                    ok, want = _copies(img, flow, cls, k)
                    m = np.broadcast_to(ok[:, None], a.shape)
                    if not np.array_equal(_bits(a)[m], _bits(want)[m]):
                        fails.append("%s %s: a zero or whole-pixel flow does not copy the input bit for bit" % (what, family))
        # frame 2 of the planar input, and bytes
        x9 = G.image_frames("gauss", B, H, W)
        flow, _ = G.warp_flow("gauss", B, H, W, k)
        f2 = ops.warp_image(hard, "input", x9, flow, k, normalized=True, frame=2)
        if not _same(f2, ops.warp_image(hard, "seq", np.ascontiguousarray(x9[:, 6:9]), flow, k, normalized=True)):
            fails.append("image warps %dx%d B %d k %g: frame 2 of the planar input is not the sequence kernel's result" % (H, W, B, k))
        xb = G.byte_frames(B, H, W, 1)
        u8 = ops.warp_image(hard, "seq", xb, flow, k)
        if not _same(u8, ops.warp_image(hard, "seq", G.unit_of_u8(xb), flow, k, normalized=False)):
            fails.append("image warps %dx%d B %d k %g: bytes do not give the bits of k / 255" % (H, W, B, k))
        v64 = G.normalize(G.unit_of_u8(xb), "64")
        fails += _check("warp-norm", "bytes", u8, G.warp(v64, flow, k, "64"), G.warp(v64, flow, k, "abs"), G.n_of("warp-norm"),
                        "warp_input_seq bytes %dx%d B %d k %g" % (H, W, B, k), row="warp-u8")
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


# ---- the first layer on a sequence -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", G.FIRST_SEQ_SHAPES, ids=lambda v: str(v))
def test_conv_first_seq(hard, H, W):
    """launch_conv_first_seq on T = 4 frames, normalized / unit / bytes, against the first layer's bound (conv_float64.ROUNDINGS['F1'],
    b2f_seq.hip:63-92); the float kinds give ops.conv_first's bits on the same frames arranged as triplets, bytes those of k / 255"""
    w, b = G.first_seq_weights()
    n = G.n_of("conv_first_seq")
    T = G.FIRST_SEQ_T
    fails = []
    for kind in ("float", "unit"):
        for family in G.FAMILIES:
            x, vals, norm = G.first_seq_case(family, H, W, kind)
            got = ops.conv_first_seq(hard, x, w, b, normalized=(kind == "float"))
            val, S = G.first_seq_reference(vals, norm, w, b)
            what = "conv_first_seq %s %dx%d" % (kind, H, W)
            fails += _check("conv_first_seq", family, got, val, S, n, what, row="first_seq-" + kind)
            x9 = np.stack([np.concatenate([x[t], x[t + 1], x[t + 2]], 0) for t in range(T - 2)])
            trip = ops.conv_first(hard, x9, w, b, normalize=norm)          # image f * B + t = frame t + f
            for f in range(3):
                for t in range(T - 2):
                    if not _same(trip[f * (T - 2) + t], got[t + f]):
                        fails.append("%s %s: frame %d is not conv_first's image (%d, %d)" % (what, family, t + f, f, t))
    x, vals, norm = G.first_seq_case("gauss", H, W, "u8")
    got = ops.conv_first_seq(hard, x, w, b)
    if not _same(got, ops.conv_first_seq(hard, vals, w, b, normalized=False)):
        fails.append("conv_first_seq %dx%d: bytes do not give the bits of k / 255" % (H, W))
    val, S = G.first_seq_reference(vals, True, w, b)
    fails += _check("conv_first_seq", "bytes", got, val, S, n, "conv_first_seq u8 %dx%d" % (H, W), row="first_seq-u8")
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", G.LAYOUT_C)
def test_layout_kernels(hard, C):
    """launch_nhwc_to_planar (pix stride C and C + 6), launch_cp8_to_planar (C no multiple of 8), launch_planar_to_nhwc: exact copies, +0 in
    the padding; the slots the kernels do not own hold NaN (b2f_glue.hip:521,542,561)"""
    fails = []
    for (h, w) in G.LAYOUT_HW:
        for family in ("gauss", "outlier", "integers"):
            x = G.field(family, (2, C, h, w), salt=40)
            for ps in (C, C + 6):
                if not _same(ops.layout(hard, "nhwc_to_planar", G.records(x, ps), C), x):
                    fails.append("nhwc_to_planar C %d ps %d %dx%d %s" % (C, ps, h, w, family))
                back = ops.layout(hard, "planar_to_nhwc", x, C, ps)
                if not (_same(back[..., :C], np.moveaxis(x, 1, 3)) and not _bits(back[..., C:]).any()):
                    fails.append("planar_to_nhwc C %d ps %d %dx%d %s" % (C, ps, h, w, family))
            if not _same(ops.layout(hard, "cp8_to_planar", G.to_cp8(x), C), x):
                fails.append("cp8_to_planar C %d %dx%d %s" % (C, h, w, family))
    assert not fails, "\n".join(fails)


# ---- the executor's node kernels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
def test_put_channels(hard, kind):
    """put_channels (b2f_graph.hip:28-42): the C channels land at c_off, every other element of the pre-filled destination keeps its bits"""
    fails = []
    B, h, w = 2, 3, 4
    for c_off in G.PUT_C_OFF:
        for C in G.PUT_C:
            for family in ("gauss", "integers"):
                src = G.field(family, (B, C, h, w), salt=30)
                dst = G.to_cp8(G.field("dc", (B, ((c_off + C + 7) // 8 + 1) * 8, h, w), salt=31)).reshape(B, -1, h * w, 8)
                arg = {0: G.to_cp8(src).reshape(B, -1, h * w, 8), 1: np.ascontiguousarray(np.moveaxis(src, 1, 3)).reshape(B, h * w, C),
                       2: src.reshape(B, C, h * w)}[kind]
                got = ops.graph_put_channels(hard, arg, kind, C, dst, c_off)
                want = G.put_channels(src, dst.reshape(B, -1, h, w, 8), c_off).reshape(dst.shape)
                if not _same(got, want):
                    fails.append("put_channels kind %d C %d c_off %d %s: %d elements differ" % (kind, C, c_off, family, int((_bits(got) != _bits(want)).sum())))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("win", G.COSTVOL_WIN)
def test_costvol_cp8(hard, win):
    """costvol_cp8 (b2f_graph.hip:47-85) with and without frmB, with and without dstS, on maps smaller than the window: each direction within
    (C + 1) u S; dstS the float32 sum of the two halves, on bits; what the kernel does not write keeps the buffer's NaN; win = 9 agrees with
    ops.costvol within the two bounds added"""
    nd = win * win
    fails = []
    for C in G.COSTVOL_C:
        for (h, w) in G.COSTVOL_HW:
            for family in G.FAMILIES:
                maps = G.costvol_maps(family, 2, C, h, w)
                ref, fF, fB = maps
                cp = [G.to_cp8(m) for m in maps]
                chJ2, chJ1, chS = (2 * nd + 7) // 8, (nd + 7) // 8, (nd + 7) // 8
                J, S_ = ops.graph_costvol(hard, cp[0], cp[1], cp[2], C, win, chJ2, chS)
                J0, none = ops.graph_costvol(hard, cp[0], cp[1], None, C, win, chJ2)
                J1, _ = ops.graph_costvol(hard, cp[0], cp[1], cp[2], C, win, chJ2)
                what = "costvol_cp8 win %d C %d %dx%d" % (win, C, h, w)
                full = G.from_cp8(J, chJ2 * 8)
                halves = {True: full[:, :nd], False: full[:, nd:2 * nd]}
                if not (_bits(full[:, 2 * nd:]) == NAN_WORD).all() or not (_bits(G.from_cp8(S_, chS * 8)[:, nd:]) == NAN_WORD).all():
                    fails.append("%s %s: a padding channel was written" % (what, family))
                if not _same(J1, J):
                    fails.append("%s %s: dstJ depends on dstS" % (what, family))
                f0 = G.from_cp8(J0, chJ2 * 8)
                if none is not None or not _same(f0[:, :nd], halves[True]) or not (_bits(f0[:, nd:]) == NAN_WORD).all():
                    fails.append("%s %s: without frmB the forward half differs or more than it was written" % (what, family))
                if not _same(G.from_cp8(S_, nd), (halves[True] + halves[False]).astype(f32)):
                    fails.append("%s %s: dstS is not the rounded sum of the two halves" % (what, family))
                for fwd, frm in ((True, fF), (False, fB)):
                    val, S = G.costvol(ref, frm, win, fwd, "64"), G.costvol(ref, frm, win, fwd, "abs")
                    fails += _check("costvol_cp8", family, halves[fwd], val, S, G.n_of("costvol_cp8", C), what + (" fwd" if fwd else " bwd"))
                    if family == "integers" and not _same(halves[fwd], val.astype(f32)):
                        fails.append("%s integers %s: not the exact result" % (what, "fwd" if fwd else "bwd"))
                    if win == 9:
                        other = ops.costvol(hard, ref, frm, 9, fwd)
                        bar = (G.n_of("costvol_cp8", C) + C + 16) * G.U * S          # + cv_float64's bar of ops.costvol's kernel
                        if not (np.abs(other.astype(f64) - halves[fwd].astype(f64)) <= bar).all():
                            fails.append("%s %s: ops.costvol differs by more than the two bounds added" % (what, family))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


@pytest.mark.parametrize("H,W", G.WARP_SHAPES, ids=lambda v: str(v))
def test_warp_cp8(hard, H, W):
    """warp_cp8 (b2f_graph.hip:89-114) on 1 and 3 chunks with the warps' flows, packed"""
    fails = []
    for chunks in (1, 3):
        for B in G.WARP_BATCHES:
            for k in G.WARP_K:
                for family in G.FAMILIES:
                    img = G.field(family, (B, chunks * 8, H, W), salt=4)
                    flow, cls = G.warp_flow(family, B, H, W, k)
                    got = G.from_cp8(ops.graph_warp(hard, G.to_cp8(img), np.ascontiguousarray(np.moveaxis(flow, 1, 3)), k), chunks * 8)
                    what = "warp_cp8 %d chunks %dx%d B %d k %g" % (chunks, H, W, B, k)
                    fails += _check("warp_cp8", family, got, G.warp(img, flow, k, "64"), G.warp(img, flow, k, "abs"), G.n_of("warp_cp8"), what)
                    if family == "integers" and not _same(got, G.warp(img, flow, k, "64").astype(f32)):
                        fails.append(what + " integers: not the exact result")
                    if cls is not None:
                        ok, want = _copies(img, flow, cls, k)
                        m = np.broadcast_to(ok[:, None], got.shape)
                        if not np.array_equal(_bits(got)[m], _bits(want)[m]):
                            fails.append("%s %s: a zero or whole-pixel flow does not copy the input bit for bit" % (what, family))
    assert not fails, "%d failures:\n" % len(fails) + "\n".join(fails)


def test_add_flow_and_scale(hard):
    """add_flow (b2f_graph.hip:118-123): one rounding, the float32 sum, slots 2..7 of the records untouched; scale by 2.0 (:126-130): exact"""
    fails = []
    for family in G.FAMILIES:
        a, b = G.field(family, (1, 2, 9, 7), salt=20), G.field(family, (1, 2, 9, 7), salt=21)
        fs, u = G.records(a, 8).reshape(-1, 8), G.records(b, 2).reshape(-1, 2)
        got = ops.graph_add_flow(hard, fs, u)
        if not _same(got[:, 2:], fs[:, 2:]):
            fails.append("add_flow %s: slots 2..7 changed" % family)
        if not _same(got[:, :2], (fs[:, :2] + u).astype(f32)):
            fails.append("add_flow %s: not the float32 sum" % family)
        val = fs[:, :2].astype(f64) + u.astype(f64)
        fails += _check("add_flow", family, got[:, :2], val, np.abs(fs[:, :2].astype(f64)) + np.abs(u.astype(f64)), G.n_of("add_flow"), "add_flow 9x7")
        p = G.field(family, (3, 2, 10, 14), salt=22)
        if not _same(ops.graph_scale(hard, p, 2.0), (p * f32(2)).astype(f32)):
            fails.append("scale %s: not exactly 2 p" % family)
    assert not fails, "\n".join(fails)
