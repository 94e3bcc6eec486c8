"""GPU: the conv kernels and the warp + cost-volume kernel in the layout the forward pass runs them in.

ops.layer (b2f_op_layer) runs one conv of a model's own packed table through run_conv: chunk-planar buffers, the two K segments and the
permuted cin_map of a first decoder layer, the record slots the layer does not read filled with non-zero numbers, the kernel chosen by
choose_kernel under the model's options.  ops.cv_record (b2f_op_cv_record) runs the cost-volume kernel on the forward's strides, with
flow_b, and returns the whole 168-slot record.  The kernel-level tests of tests/test_gpu_parity.py run the same kernels on NHWC strides,
one segment and an identity map.

Expected values: a float64 convolution (torch, CPU) of the layer's Torch weights and Torch-order input; the oracle's composition of
test_warp_costvol_fused.  Bars: the ones tests/test_gpu_parity.py holds the kernel that ran to (BARS below names the test each comes
from); the kernel that ran is read from the profile rows and must be the one the setting names."""
import functools

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops, weights as W
from oracle import oracle as O
from tests.layer_models import BIG, SETTINGS, flat as _flat, name as _name, open_model  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FEAT = W.FEAT
SIZES = [(1, 1), (8, 16), (17, 33), (24, 40)]     # of the output: smallest; one F(2x2) tile; one past an F(4x4) block both ways, ragged for 6 x 6 tiles; a level of the forward
HOLE_SIZE = (17, 33)

WIDE = ["default", "f4x4", "f6x6", "wino1d-1", "wino1d-2", "bf16-wide", "f2x2-split", "adaptive"]      # stride 1, >= 32 outputs: the F(4x4) class
STRIDE2 = ["default", "bf16_conv-0", "s2_loader-0", "s2_loader-2", "s2_tile_groups-0", "s2_tiles_per_block-2"]
FIXED = ["default"]                                                                                   # 16 -> 16, 16 -> 32, 32 -> 2: one kernel each


def _allclose(rtol, atol, mean=None, worst=None):
    def check(got, exp, what):
        err = np.abs(got - exp)
        np.testing.assert_allclose(got, exp, rtol=rtol, atol=atol, err_msg=what)
        if mean is not None:
            assert err.mean() < mean, (what, float(err.mean()))
        if worst is not None:
            assert err.max() <= worst, (what, float(err.max()))
    return check


# the bar of each kernel, by its profile tag (kKernels, csrc/b2f_api.hip)
BARS = {
    "D1": _allclose(2e-5, 2e-5), "D2": _allclose(2e-5, 2e-5), "C16": _allclose(2e-5, 2e-5), "S16": _allclose(2e-5, 2e-5),
    "N2": _allclose(2e-5, 2e-5),                                    # test_conv3x3: direct, 16-channel and two-output kernels
    "W4": _allclose(1e-4, 1.5e-4, mean=5e-6),                       # test_conv3x3
    "W6": _allclose(1e-4, 1.5e-4, mean=5e-6),                       # test_conv3x3_wino6
    "W2": _allclose(2e-5, 3e-5),                                    # test_conv3x3_f2x2_one_n_tile_per_block (up to 264 input channels)
    "W2+": _allclose(2e-5, 1e-4),                                   # test_conv3x3_wino_eight_wave_form_bit_identical (more input channels, up to 562)
    "E1": _allclose(1e-4, 1e-4, mean=5e-6, worst=1e-4),             # test_direct_conv_on_the_bf16_pipe: max <= 1e-4, mean < 5e-6 against float64
    "E2": _allclose(1e-4, 1e-4, mean=5e-6, worst=1e-4),
    "L2": _allclose(2e-5, 2e-5, worst=1e-4),                        # test_stride2_loader_consumer_kernel
    "V1": _allclose(1e-4, 5e-5),                                    # test_conv3x3_one_dimensional_winograd_on_the_bf16_pipe
}


def _expected_tags(cls, setting, co):
    if cls == "fixed":
        return None
    if cls == "s2":
        return {"default": None, "bf16_conv-0": {"D2"}, "s2_loader-0": {"E2"}, "s2_loader-2": {"L2"}, "s2_tile_groups-0": {"L2"},
                "s2_tiles_per_block-2": {"D2"}}[setting]
    w1 = co // 64 + (1 if co % 64 > 32 else 0)                     # wino1d = 1: n-blocks of more than 32 real outputs
    return {"default": {"W2"}, "f4x4": {"W4"}, "f6x6": {"W6"}, "wino1d-1": {"V1"} if w1 else {"W4"}, "wino1d-2": {"V1"}, "bf16-wide": {"E1"},
            "f2x2-split": {"W2"}, "adaptive": {"W2", "W4"}}[setting]


# ---- models: one context per (kind, setting), alive for the module ----

_MODELS = {}


def _model(which, setting):
    key = (which, setting)
    if key not in _MODELS:
        _MODELS[key] = open_model(which, setting)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _ran(m, call):
    """(result of call(), the tag of the one conv row the call left in the profile)"""
    m.profile_reset()
    out = call()
    rows = [n for n, (ms, cnt) in m.profile_read().items() if cnt > 0 and n.startswith("conv")]
    assert len(rows) == 1, rows
    return out, rows[0][4:].split("_")[0]


# ---- layers ----

def _layers():
    """(id, kind of model, kind, level, idx, class)"""
    out = []
    for l in range(2, 8):
        for idx in (1, 2):
            if (l, idx) == (2, 1):
                continue                                           # launch_conv_first, not run_conv
            cls = "fixed" if l == 2 or (l == 3 and idx == 1) else ("s2" if idx == 1 else "wide")
            out.append(("hard", "feat", l, idx, cls))
    for which, kinds in (("hard", ("occ", "flow")), ("soft", ("occ", "flow", "past"))):
        for l in range(3, 8):
            for kind in kinds:
                out.append((which, kind, l, 1, "wide"))
    for which, kind, l in (("hard", "occ", 3), ("hard", "flow", 5), ("soft", "past", 7)):
        for idx in range(2, 7):
            out.append((which, kind, l, idx, "fixed" if idx == 6 else "wide"))
    return out


def _float64(x, wt, b, stride, leaky):
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1, stride=stride)
    return (torch.where(y > 0, y, 0.2 * y) if leaky else y).numpy()


@pytest.mark.parametrize("which,kind,level,idx,cls", _layers(), ids=lambda v: str(v))
def test_layer_in_the_forwards_layout(which, kind, level, idx, cls):
    """One conv of the model at every size under every setting that can change its kernel: the float64 convolution at the bar of the kernel
    that ran; that kernel is the one the setting names; a one-segment layer gives the bits of ops.conv3x3 under the same options (the same
    kernel on other addresses); a first decoder layer gives the same bits when the record slots it does not read hold other numbers."""
    past = which == "soft"
    v = W.views(_flat(which), past)
    wt, b = v[_name(kind, level, idx) + ".w"], v[_name(kind, level, idx) + ".b"]
    co, ci = wt.shape[:2]
    stride = 2 if (kind == "feat" and idx == 1) else 1
    leaky = kind == "feat" or idx < 6
    first = kind != "feat" and idx == 1
    nimg = 2 + level % 2
    r = np.random.default_rng(1000 * level + 10 * idx + len(kind))
    failures = []                                                  # every size and setting runs; one assertion at the end names all that failed
    for Ho, Wo in SIZES:
        x = r.standard_normal((nimg, ci, Ho * stride, Wo * stride), dtype=np.float32)      # flow channels included
        exp = _float64(x, wt, b, stride, leaky)
        for setting in {"wide": WIDE, "s2": STRIDE2, "fixed": FIXED}[cls]:
            what = "%s %s %dx%d %s" % (which, _name(kind, level, idx), Ho, Wo, setting)
            try:
                _check_layer(_model(which, setting), kind, level, idx, cls, setting, x, wt, b, exp, stride, leaky, first, (Ho, Wo) == HOLE_SIZE, what)
            except AssertionError as e:
                failures.append("%s: %s" % (what, str(e).strip()[:600]))
    assert not failures, "%d of the cases failed:\n" % len(failures) + "\n".join(failures)


def _check_layer(m, kind, level, idx, cls, setting, x, wt, b, exp, stride, leaky, first, holes, what):
    co, ci = wt.shape[:2]
    got, tag = _ran(m, lambda: ops.layer(m, kind, level, idx, x))
    assert got.shape == exp.shape and np.isfinite(got).all(), what
    tags = _expected_tags(cls, setting, co)
    assert tags is None or tag in tags, (what, tag, tags)
    bar = "W2+" if (tag == "W2" and ci > 264) else tag
    print("layer %-46s ran %-3s max|gpu - float64| = %.3g mean %.3g" % (what, tag, float(np.abs(got - exp).max()), float(np.abs(got - exp).mean())))
    BARS[bar](got, exp, what + " ran " + tag)
    # ops.conv3x3 chooses by the same options.  Only for the F(4x4) class does it differ from the forward: it leaves the small-map fallback to
    # F(2x2) and the per-launch rule out, so those layers are compared under the settings that name their kernel; option op_wino_split = 1
    # puts its layers of more than 32 outputs on that fallback, split as wino_split_pixels splits them here.  Every other layer has one rule.
    comparable = cls != "wide" or (setting not in ("default", "adaptive") and (setting != "f2x2-split" or co > 32))
    if not first and comparable:
        with m.options(op_wino_split=int(setting == "f2x2-split")):
            same = ops.conv3x3(m, x, wt, b, stride, leaky)
        np.testing.assert_array_equal(got, same, err_msg=what + ": not the bits of ops.conv3x3 on " + tag)
    if first and holes:
        with m.options(op_hole_fill=7):
            again = ops.layer(m, kind, level, idx, x)
        np.testing.assert_array_equal(got, again, err_msg=what + ": the result depends on record slots the layer does not read")


def test_layer_entry_refuses_what_it_does_not_cover():
    m = _model("hard", "default")
    x = np.zeros((1, 3, 8, 8), np.float32)
    with pytest.raises(_lib.B2FError, match="launch_conv_first"):
        ops.layer(m, "feat", 2, 1, x)
    with pytest.raises(_lib.B2FError, match="no conv"):
        _lib.check(_lib.lib().b2f_op_layer(m._h, 3, 5, 1, 1, 8, 8, _lib.fptr(x), _lib.fptr(x)))   # Hard: no past-flow decoder


# ---- records ----

SLOT = lambda d, c: c if (d == 0 and c < 80) else (80 + c if c < 80 else 160 + d)      # cv_slot of csrc/b2f_internal.h
REC_K = {32: 5.0, 64: 2.5, 96: 1.25, 128: 0.625, 192: 0.625}
PRODUCT_VARIANTS = [0, 1, 3, 5, 7]


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


def _flows(r, B, h, w):
    """the flows of test_warp_costvol_fused (noise and two points through the clamp) and a translation of several pixels plus noise"""
    a = (r.standard_normal((B, 2, h, w)) * 0.8).astype(np.float32)
    a[0, :, 0, 0] = (-30, -30)
    a[0, :, h - 1, w - 1] = (30, 30)
    t = (r.uniform(-6, 6, (B, 2, 1, 1)) + 0.15 * r.standard_normal((B, 2, h, w))).astype(np.float32)
    return {"noise": a, "translation": t}


def _record_case(C, h, w):
    r = np.random.default_rng(C * 7 + h)
    B = 2
    maps = [r.standard_normal((B, C, h, w), dtype=np.float32) for _ in range(3)]       # ref, future, past
    flows = _flows(r, B, h, w)
    flows_b = {n: (f[:, ::-1] * np.float32(-0.7) + np.float32(0.25)).astype(np.float32) for n, f in flows.items()}
    return maps, flows, flows_b


def _check_record(rec, maps, flow, flow_b, k, what):
    ref, f3, f1 = maps
    w3 = O.warping_unit(f3, flow, k) if flow is not None else f3
    w1 = O.warping_unit(f1, flow, -k) if flow is not None else f1
    exp = np.concatenate([O.costvol([ref, w3], 9, True), O.costvol([ref, w1], 9, False)], 1)
    slots = [SLOT(d, c) for d in (0, 1) for c in range(81)]
    assert sorted(slots) == list(range(162))
    err = float(np.abs(rec[:, slots] - exp).max())
    print("record %-44s max|gpu - oracle| = %.3g" % (what, err))
    np.testing.assert_allclose(rec[:, slots], exp, rtol=1e-4, atol=5e-6, err_msg=what)
    zero = np.zeros_like(rec[:, :2])
    np.testing.assert_array_equal(rec[:, 162:164], flow if flow is not None else zero, err_msg=what + ": slots 162 / 163")
    np.testing.assert_array_equal(rec[:, 164:166], flow_b if flow_b is not None else zero, err_msg=what + ": slots 164 / 165")
    np.testing.assert_array_equal(rec[:, 166:168], zero, err_msg=what + ": slots 166 / 167")


def _record_configs(flows, flows_b):
    yield "no flow", None, None
    for n in flows:
        yield n, flows[n], None
        yield n + " + flow_b", flows[n], flows_b[n]


@pytest.mark.parametrize("h,w", [(1, 2), (9, 17), (16, 30), (24, 40)])
@pytest.mark.parametrize("C", [32, 64, 96, 128, 192])
def test_record_in_the_forwards_layout(hard, C, h, w):
    """The whole record on chunk-planar strides: the 162 cost-volume slots against the oracle's composition (variant 3), the flow slots
    exactly flow and flow_b (0 where the pointer is NULL), slots 166 / 167 exactly 0 -- and every product variant the bits of variant 3."""
    maps, flows, flows_b = _record_case(C, h, w)
    k = REC_K[C]
    for name, flow, flow_b in _record_configs(flows, flows_b):
        what = "C %d %dx%d k %g %s" % (C, h, w, k, name)
        with hard.options(corr_variant=3):
            base = ops.cv_record(hard, *maps, flow, flow_b, k)
        _check_record(base, maps, flow, flow_b, k, what)
        for variant in PRODUCT_VARIANTS:
            with hard.options(corr_variant=variant):
                rec = ops.cv_record(hard, *maps, flow, flow_b, k)
            np.testing.assert_array_equal(rec, base, err_msg="%s: variant %d is not variant 3" % (what, variant))
        with hard.options(corr_variant=-1):
            rec = ops.cv_record(hard, *maps, flow, flow_b, k)
        np.testing.assert_array_equal(rec, base, err_msg=what + ": the automatic choice is not variant 3")


@pytest.mark.parametrize("variant", [2, 4, 6, 8])
def test_record_experiment_variants(hard, variant):
    if not hard.get_option("experiments"):      # the check of tests/test_gpu_parity.py: these kernels live in tools/experiments/csrc
        pytest.skip("experiment kernel: not in the product library (python -m back2future_amd.build --experiments; B2F_LIB=back2future_amd/libb2f_exp.so)")
    for C, (h, w) in ((32, (24, 40)), (64, (16, 30)), (96, (9, 17)), (128, (1, 2)), (192, (9, 17))):
        maps, flows, flows_b = _record_case(C, h, w)
        for name, flow, flow_b in _record_configs(flows, flows_b):
            with hard.options(corr_variant=3):
                base = ops.cv_record(hard, *maps, flow, flow_b, REC_K[C])
            with hard.options(corr_variant=variant):
                rec = ops.cv_record(hard, *maps, flow, flow_b, REC_K[C])
            np.testing.assert_array_equal(rec, base, err_msg="C %d %dx%d %s: variant %d is not variant 3" % (C, h, w, name, variant))
