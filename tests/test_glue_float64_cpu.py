"""CPU: tests/glue_float64.py against itself, before any kernel is held to it.

Each float64 reference agrees with an independent witness on the GPU file's own shapes and families (torch's align-corners bilinear
interpolation, tests/torch_ref.py's gather, torch's average pooling and softmax, tests/cv_float64.py's cost volume); the float32 emulation
of each kernel stays inside the counted bound on every family and its worst err / (2^-24 S) is the recorded table
(tests/golden/glue_float64_ratios.json) the GPU file reads; every mutation of the emulation turns the bound red on those inputs; the cases
whose `integers` results are exact are derived here."""
import numpy as np
import pytest
import torch

from tests import cv_float64 as CV
from tests import glue_float64 as G
from tests import torch_ref as TR

f32, f64 = np.float32, np.float64
WILD = ("gauss", "dc", "ramp", "outlier")          # the families a mutation must turn red on


def test_version():
    from back2future_amd import _lib, build
    build.build()
    assert _lib.lib().b2f_version() >= 1009


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", G.UPSAMPLE_SHAPES)
def test_upsample_reference_against_torch(h, w):
    """F.interpolate(align_corners=True) in float64 computes the cell from a double ratio; where the kernel's float32 cast lands in another
    cell the two are not compared, and those outputs are at most 1 % of a case.  Elsewhere the weights differ by the rounding of
    r and r * i (<= 2 u c each axis), so the values agree within 8 u max(2h, 2w) max |x|."""
    for family in G.FAMILIES:
        for B in G.UPSAMPLE_BATCHES:
            x, val, S = G.upsample_case(family, B, h, w)
            want = torch.nn.functional.interpolate(torch.from_numpy(x.astype(f64)), scale_factor=2, mode="bilinear", align_corners=True).numpy()
            same = []
            for n in (h, w):
                cell64 = np.floor((n - 1) / (2 * n - 1) * np.arange(2 * n)).astype(np.int64) if n > 1 else np.zeros(2 * n, np.int64)
                same.append(G.up_axis(n)[0] == cell64)
            ok = same[0][:, None] & same[1][None, :]
            assert (~ok).mean() <= 0.01, (family, B, h, w, float((~ok).mean()))
            tol = 8 * G.U * max(2 * h, 2 * w) * float(np.abs(x).max()) + 1e-12
            assert np.abs(val - want)[:, :, ok].max() <= tol, (family, B, h, w)
            assert (np.abs(val) <= S * (1 + 1e-12)).all()


@pytest.mark.parametrize("h,w", G.UPSAMPLE_SHAPES)
def test_upsampling_a_ramp_gives_the_ramp(h, w):
    """bilinear x2 of a linear field is the field at c = r * i (c - i1 is exact): the reference differs from it by the rounding of the
    float32 samples and of l0 = 1 - l1 on each axis, 3/2 u S, inside the kernel's bound of 4 u S"""
    for B in G.UPSAMPLE_BATCHES:
        x, val, S = G.upsample_case("ramp", B, h, w)
        pos = lambda n: (f32(n - 1) / f32(2 * n - 1) * np.arange(2 * n, dtype=f32)).astype(f32)
        want = G.ramp((B, 2, h, w), 0, pos(h), pos(w))
        assert G.measure(val, want, S) <= G.n_of("upsample")


def _warp_inputs(family, B, H, W, k):
    return G.image_frames(family, B, H, W)[:, :3], G.warp_flow(family, B, H, W, k)


@pytest.mark.parametrize("H,W", G.WARP_SHAPES)
def test_warp_reference_against_the_gather_witness(H, W):
    """tests/torch_ref.warp_gather computes positions in float64.  On the `integers` flows every position is exact in both arithmetics: the
    two agree to float64 rounding.  On the mixed flows the float32 position is off by at most 2 u |c| <= 2^-17 pixels below |c| = 64, which
    moves a blend by at most that times twice the largest sample (the +-1e6 targets clamp in both)."""
    for family in G.FAMILIES:
        for B in G.WARP_BATCHES:
            for k in G.WARP_K:
                img, (flow, _) = _warp_inputs(family, B, H, W, k)
                val = G.warp(img, flow, k, "64")
                want = TR.warp_gather(torch.from_numpy(img.astype(f64)), torch.from_numpy(flow.astype(f64) * k)).numpy()
                top = float(np.abs(img).max())
                tol = 1e-12 * top if family == "integers" else 2.0 ** -16 * top
                assert np.abs(val - want).max() <= tol, (family, B, H, W, k, float(np.abs(val - want).max()))
                assert (np.abs(val) <= G.warp(img, flow, k, "abs") * (1 + 1e-12)).all()


def test_avgpool_and_softmax_references_against_torch():
    for (H, W) in G.AVGPOOL_SHAPES:
        for family in G.FAMILIES:
            x = G.avgpool_input(family, 2, H, W)
            want = torch.nn.functional.avg_pool2d(torch.from_numpy(np.moveaxis(x, 3, 1).astype(f64)), 2).numpy()
            assert np.abs(np.moveaxis(G.avgpool(x, "64"), 3, 1) - want).max() <= 1e-12 * np.abs(x).max()
    for (h, w) in G.SOFTMAX_SHAPES:
        z, cls = G.softmax_logits(2, h, w)
        p = G.softmax(z, "64")
        want = torch.softmax(torch.from_numpy(z.astype(f64)), 1).numpy()
        # z - m is rounded to float32 first (the operand of expf): |z - m| <= 208 moves exp by 208 u relative
        assert np.abs(p - want).max() <= 1e-4 and (np.abs(p - want) <= 1e-4 * want + 1e-300).all()
        assert (p[:, 0][cls >= 6] == 0.5).all() and (p[:, 1][cls >= 6] == 0.5).all()
        assert {2, 3, 4, 5} <= set(np.unique(G.softmax_logits(2, 2, 257)[1]))


@pytest.mark.parametrize("win", G.COSTVOL_WIN)
def test_costvol_reference_against_cv_float64(win):
    for C in G.COSTVOL_C:
        for (h, w) in G.COSTVOL_HW:
            for family in ("gauss", "integers"):
                ref, fF, fB = G.costvol_maps(family, 2, C, h, w)
                for fwd, frm in ((True, fF), (False, fB)):
                    val, S = CV.costvol64(ref, frm, win, fwd)
                    assert np.abs(G.costvol(ref, frm, win, fwd, "64") - val).max() <= 1e-12 * max(1.0, np.abs(val).max())
                    assert np.abs(G.costvol(ref, frm, win, fwd, "abs") - S).max() <= 1e-12 * max(1.0, S.max())
                    want = TR.costvol_lua(torch.from_numpy(ref.astype(f64)), torch.from_numpy(frm.astype(f64)), win, fwd).numpy()
                    assert np.abs(val - want).max() <= 1e-12 * max(1.0, np.abs(val).max())


def test_layout_helpers_round_trip():
    x = G.field("gauss", (2, 13, 3, 5))
    cp = G.to_cp8(x)
    assert cp.shape == (2, 2, 3, 5, 8) and np.array_equal(G.from_cp8(cp, 13), x) and np.isnan(cp[:, 1, :, :, 5:]).all()
    rec = G.records(x[:, :2], 8)
    assert np.array_equal(rec[..., 0], x[:, 0]) and np.array_equal(rec[..., 1], x[:, 1]) and np.isnan(rec[..., 2:]).all()
    dst = G.to_cp8(G.field("dc", (2, 24, 3, 5)), 0.0)
    out = G.put_channels(x, dst, 9)
    assert np.array_equal(G.from_cp8(out, 24)[:, 9:22], x) and np.array_equal(G.from_cp8(out, 24)[:, :9], G.from_cp8(dst, 24)[:, :9])
    assert np.array_equal(G.from_cp8(out, 24)[:, 22:], G.from_cp8(dst, 24)[:, 22:])


# ---- the emulation: inside the bound, and the recorded table --------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", G.EMULATED + ("softmax",))
def test_emulation_meets_the_bound_and_is_the_recorded_table(kernel):
    fails = []
    for family in (("logits",) if kernel == "softmax" else G.families_of(kernel)):
        ratio, frac = G.emulation_ratios(kernel, "gauss" if family == "bytes" else family)
        n = 0 if kernel == "softmax" else G.n_of(G.BOUND_OF.get(kernel, kernel))
        print("%-16s %-8s worst err / (u S) = %8.3f  worst err / bound = %.3f (n = %s)" % (kernel, family, ratio, frac, "2 E + 3" if kernel == "softmax" else "%d%s" % (n, " + C" if kernel == "costvol_cp8" else "")))
        if not frac <= 1.0:
            fails.append("%s %s: the emulation is at %.3f of the bound" % (kernel, family, frac))
        rec = G.recorded(kernel, family)
        if not abs(ratio - rec) <= 1e-3 * rec + 1e-9:
            fails.append("%s %s: worst ratio %.6g, recorded %.6g (python -m tests.glue_float64 rewrites the file)" % (kernel, family, ratio, rec))
    assert not fails, "\n".join(fails)


def test_the_recorded_table_has_no_other_rows():
    assert set(G.recorded_ratios()) == set(G.EMULATED) | {"softmax"}


# ---- mutations ----------------------------------------------------------------------------------------------------------------------------

MUTATIONS = [("upsample", "ratio"),                 # h / H2 where (h - 1) / (H2 - 1) belongs
             ("upsample", "noclamp"),               # the + 1 neighbour of the last row / column wraps
             ("upsample", "swap-scalar"), ("upsample", "swap-vector"),          # u and v swapped on one of the two store paths
             ("upsample", "tail"),                  # the tail group's min(x0 + k, W2 - 1) off by one
             ("warp", "frac"), ("warp-norm", "frac"), ("warp_cp8", "frac"),     # top-left weight frac instead of 1 - frac
             ("warp", "sign"), ("warp-norm", "sign"), ("warp_cp8", "sign"),     # k with the wrong sign
             ("avgpool", "tap"),                    # one pool tap dropped
             ("costvol_cp8", "transpose"),          # qx / qy transposed
             ("costvol_cp8", "bwd-y"),              # the backward direction read at y - qy
             ("first_seq-unit", "pad")]             # ColorNormalize applied after the zero padding


@pytest.mark.parametrize("kernel,mutate", MUTATIONS)
def test_a_mutated_emulation_breaks_the_bound(kernel, mutate):
    for family in WILD:
        _, frac = G.emulation_ratios(kernel, family, mutate)
        print("%-16s %-12s %-8s worst err / bound = %.3g" % (kernel, mutate, family, frac))
        assert frac > 1.0, "%s with mutation %s stays inside the bound on %s (%.3f): the inputs are too tame" % (kernel, mutate, family, frac)


def test_the_byte_and_softmax_and_copy_mutations_break_their_checks():
    assert G.emulation_ratios("first_seq-u8", "gauss", "pad")[1] > 1.0
    assert G.emulation_ratios("warp-u8", "gauss", "sign")[1] > 1.0 and G.emulation_ratios("warp-u8", "gauss", "frac")[1] > 1.0
    assert G.emulation_ratios("softmax", "logits", "planes")[1] > 1.0                      # the two planes swapped
    for family in G.FAMILIES:                                                                 # put_channels with c_off rounded down to 8
        for c_off in G.PUT_C_OFF:
            src, dst = G.field(family, (2, 2, 3, 4), salt=30), G.to_cp8(G.field(family, (2, 96, 3, 4), salt=31), 0.0)
            same = np.array_equal(G.put_channels(src, dst, c_off, "c_off8"), G.put_channels(src, dst, c_off))
            assert same == (c_off % 8 == 0), (family, c_off)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------

def _exact(emu32, val64):
    return bool(np.array_equal(val64.astype(f32).astype(f64), val64) and np.array_equal(emu32, val64.astype(f32)))


def test_the_exact_upsample_cases_are_the_listed_ones():
    """`integers`: the shapes at which the float64 reference is a float32 array and the emulation reproduces it, both batches"""
    exact = [(h, w) for (h, w) in G.UPSAMPLE_SHAPES
             if all(_exact(G.upsample(G.upsample_case("integers", B, h, w)[0], "32"), G.upsample_case("integers", B, h, w)[1]) for B in G.UPSAMPLE_BATCHES)]
    assert exact == G.UPSAMPLE_EXACT


def test_integers_are_exact_where_the_gpu_file_asserts_bits():
    """warps on `integers` images and flows without ColorNormalize, the pool, add_flow: the reference is a float32 array and the emulation
    gives it; the executor's cost volume: the sum of products is exact and the one division is the reference rounded once"""
    for (H, W) in G.WARP_SHAPES:
        for B in G.WARP_BATCHES:
            for k in G.WARP_K:
                img, (flow, _) = _warp_inputs("integers", B, H, W, k)
                assert _exact(G.warp(img, flow, k, "32"), G.warp(img, flow, k, "64")), (H, W, B, k)
    for (H, W) in G.AVGPOOL_SHAPES:
        x = G.avgpool_input("integers", 6, H, W)
        assert _exact(G.avgpool(x, "32"), G.avgpool(x, "64"))
    for C in G.COSTVOL_C:
        ref, fF, _ = G.costvol_maps("integers", 2, C, 9, 7)
        assert np.array_equal(G.costvol(ref, fF, 5, True, "32"), G.costvol(ref, fF, 5, True, "64").astype(f32))


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------

def test_every_kernel_of_the_three_files_has_an_op_level_case():
    """every __global__ function of b2f_glue.hip, b2f_seq.hip and b2f_graph.hip is named in the GPU file's map, and what the map names exists"""
    import os
    import re
    from tests import test_gpu_glue_float64 as T
    csrc = os.path.join(G.ROOT, "back2future_amd", "csrc")
    kernels = set()
    for name in ("b2f_glue.hip", "b2f_seq.hip", "b2f_graph.hip"):
        kernels |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(csrc, name)).read(), flags=re.S))
    assert len(kernels) >= 22 and kernels == set(T.KERNEL_CASES), sorted(kernels ^ set(T.KERNEL_CASES))
    for kernel, test in T.KERNEL_CASES.items():
        assert hasattr(T, test) or test.startswith(("tests/", "excepted")), (kernel, test)
    ops_src = open(os.path.join(G.ROOT, "back2future_amd", "ops.py")).read()
    for entry in ("upsample_flow2x_ex", "softmax_nearest4", "avgpool2", "pack_input", "warp_image", "conv_first_seq", "layout", "expf", "graph_put_channels",
                  "graph_costvol", "graph_warp", "graph_add_flow", "graph_scale", "graph_softmax_nearest"):
        assert "b2f_op_" + entry in ops_src, entry
