"""CPU: the recipe that compiles the reference's own bilinear sampler (oracle/reference.py) and the float64 restatement the GPU file
tests/test_gpu_reference_sampler.py holds it, the oracle and the library to (tests/sampler_float64.py).

The restatement is checked against torch.autograd through tests/torch_ref.warp_gather (as tests/test_backward_cpu.py checks the oracle),
against glue_float64.warp, and against a loop over pixels written from the reference's text; the CPU oracle already has to sit inside the
counted bounds here, and three wrong samplers -- weights exchanged, floor before clamp, the gradient's components stored y first -- must
not.  The grids have to reach what they are named for."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import reference as REF
from tests import glue_float64 as GF
from tests import sampler_float64 as SF
from tests import torch_ref as R

f32, f64 = np.float32, np.float64
ROOT = GF.ROOT
SAME_SIZE = [c for c in SF.CASES if c[1:3] == c[3:5]]


# ---- the recipe ----------------------------------------------------------------------------------------------------------------------------

def test_build_makes_both_libraries_with_the_three_entries():
    if not os.path.exists(os.path.join(REF.reference_dir(), REF.SAMPLER_DIR, REF.SAMPLER)):
        pytest.skip("no reference checkout at %s" % REF.reference_dir())
    assert REF.build() == REF.lib_path()
    for fma in (False, True):
        assert os.path.exists(REF.lib_path(fma))
        lib = ctypes.CDLL(REF.lib_path(fma))
        for entry in REF.ENTRIES:
            assert hasattr(lib, entry), (REF.lib_path(fma), entry)
    newest = max(os.path.getmtime(p) for p in REF._sources())
    assert all(os.path.getmtime(REF.lib_path(fma)) >= newest for fma in (False, True))


def test_build_without_a_checkout_uses_what_is_there(monkeypatch, tmp_path):
    monkeypatch.setenv("B2F_REFERENCE_DIR", str(tmp_path / "absent"))
    have = all(os.path.exists(REF.lib_path(fma)) for fma in (False, True))
    assert REF.build() == (REF.lib_path() if have else None)
    monkeypatch.setattr(REF, "OUT", str(tmp_path / "empty"))
    assert REF.build() is None


def test_nothing_of_the_reference_is_tracked():
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
    p = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    if p.returncode == 0:          # a git checkout: nothing under oracle/_ref/ is in the index
        assert p.stdout.decode().split() == []
    # the committed side of the recipe names the reference's file and holds none of its kernels
    for name in ("ref_sampler.cpp", os.path.join("shim", "lua.h"), os.path.join("shim", "THCGeneral.h")):
        text = open(os.path.join(REF.SRC, name)).read()
        assert "__global__" not in text and "getTopLeft" not in text, name
    assert '#include "%s"' % REF.SAMPLER in open(REF.DRIVER).read()


# ---- the counts ------------------------------------------------------------------------------------------------------------------------------

def test_counts():
    """m + 9 with m = ceil(C / 32), K + 1, 5: the figures of the helper's head"""
    assert [SF.n_grid(C) for C in (1, 3, 8, 32, 33, 40, 64, 65, 128)] == [10, 10, 10, 10, 11, 11, 11, 12, 13]
    assert SF.n_image(np.array([0, 1, 2, 58])).tolist() == [0, 2, 3, 59]
    assert SF.N_FORWARD == GF.n_of("warp_cp8") == 5
    assert SF.U == 2.0 ** -24 and SF.B == 2
    assert SF.CASES == [(3, 1, 1, 1, 1), (1, 1, 16, 1, 16), (32, 3, 17, 3, 17), (40, 7, 33, 7, 33), (33, 2, 48, 2, 48), (128, 6, 5, 6, 5),
                        (8, 5, 9, 4, 20)]


# ---- the fields ------------------------------------------------------------------------------------------------------------------------------

REQUIRED = ("clamps left", "clamps right", "clamps top", "clamps bottom", "on column 0", "on the last column", "on row 0", "on the last row",
            "top-left tap on the last column", "top-left tap on the last row", "both weights 1", "a weight inside (0, 1) on x",
            "a weight inside (0, 1) on y")
PAIRED = ("an edge on x under a blend on y", "an edge on y under a blend on x")


@pytest.mark.parametrize("case", SF.CASES, ids=SF.case_id)
def test_fields_reach_what_they_are_named_for(case):
    C, ih, iw, gh, gw = case
    for field in SF.FIELDS:
        g = SF.grid(field, case)
        assert g.dtype == f32 and g.shape == (SF.B, gh, gw, 2) and np.isfinite(g).all()
    facts = SF.field_facts(case)
    if ih > 1 and iw > 1:
        assert [k for k in REQUIRED if not facts[k]] == []
        if SF.B * gh * gw >= 100:          # every pair of the six classes occurs at least twice
            assert [k for k in PAIRED if not facts[k]] == []
    elif iw > 1:                            # one row: everything the x axis can reach
        assert [k for k in REQUIRED if "y" not in k and "row" not in k and "top" not in k and "bottom" not in k and not facts[k]] == []
    whole = SF.grid("whole", case)
    assert np.array_equal(whole, np.round(whole)) and np.signbit(whole[whole == 0]).any()
    far = np.abs(SF.grid("far", case))
    assert (far == max(ih, iw, gh, gw) + 5).all()
    c = SF.cells(SF.grid("far", case), ih, iw)
    assert ((c["xw"] == 1) & (c["yw"] == 1)).all()
    if gh * gw >= 2:
        assert len({(a, b) for a, b in zip(np.sign(SF.grid("far", case)[..., 0]).ravel(), np.sign(SF.grid("far", case)[..., 1]).ravel())}) >= 2
    c = SF.cells(SF.grid("frac", case), ih, iw)
    if iw > 1:
        assert ((c["xw"] > 0) & (c["xw"] < 1)).any()


# ---- the restatement against three witnesses ---------------------------------------------------------------------------------------------------

def _loops(img, grid, grad_out):
    """the reference's text pixel by pixel in float64 (weights from float32 coordinates): forward, image gradient, grid gradient"""
    Bn, ih, iw, C = img.shape
    _, gh, gw, _ = grid.shape
    out = np.zeros((Bn, gh, gw, C)); gi = np.zeros(img.shape); gg = np.zeros(grid.shape)

    def top_left(v, pos, size):
        c = f32(v) + f32(pos)
        c = f32(0) if c < 0 else c
        c = f32(size - 1) if c > size - 1 else c
        p = int(np.floor(c))
        return p, float(f32(1) - (c - f32(p)))

    for b in range(Bn):
        for y in range(gh):
            for x in range(gw):
                xl, xw = top_left(grid[b, y, x, 0], x, iw)
                yt, yw = top_left(grid[b, y, x, 1], y, ih)
                ux, uy = float(f32(1) - f32(xw)), float(f32(1) - f32(yw))
                go = grad_out[b, y, x].astype(f64)
                dots = {}
                for name, (yy, xx, w) in {"tl": (yt, xl, xw * yw), "tr": (yt, xl + 1, ux * yw), "bl": (yt + 1, xl, xw * uy),
                                          "br": (yt + 1, xl + 1, ux * uy)}.items():
                    dots[name] = 0.0
                    if 0 <= xx <= iw - 1 and 0 <= yy <= ih - 1:
                        out[b, y, x] += w * img[b, yy, xx].astype(f64)
                        gi[b, yy, xx] += w * go
                        dots[name] = float((img[b, yy, xx].astype(f64) * go).sum())
                gg[b, y, x, 1] = -xw * dots["tl"] + xw * dots["bl"] - ux * dots["tr"] + ux * dots["br"]
                gg[b, y, x, 0] = -yw * dots["tl"] + yw * dots["tr"] - uy * dots["bl"] + uy * dots["br"]
    return out, gi, gg


@pytest.mark.parametrize("case", [SF.CASES[0], SF.CASES[2], SF.CASES[6]], ids=SF.case_id)
def test_float64_against_loops_over_pixels(case):
    for field in SF.FIELDS:
        Rf = SF.reference(case, field)
        out, gi, gg = _loops(Rf["img"], Rf["grid"], Rf["grad_out"])
        np.testing.assert_allclose(Rf["fwd"][0], out, rtol=0, atol=1e-13 * max(1.0, float(Rf["fwd"][1].max())))
        np.testing.assert_allclose(Rf["gi"][0], gi, rtol=0, atol=1e-13 * max(1.0, float(Rf["gi"][1].max())))
        np.testing.assert_allclose(Rf["gg"][0], gg, rtol=0, atol=1e-13 * max(1.0, float(Rf["gg"][1].max())))
        assert (Rf["gi"][1][Rf["gi"][2] == 0] == 0).all()          # S = 0 where nothing lands


@pytest.mark.parametrize("case", SAME_SIZE, ids=SF.case_id)
def test_float64_against_autograd(case):
    """grids in odd eighths of a pixel: every coordinate is exact in float32 and in float64 and none sits on a kink, so torch's float64
    gather sees the cells the restatement sees.  Image gradient everywhere; grid gradient on the interior (autograd differentiates the
    clamp, the reference's lines 287-288 do not)."""
    C, ih, iw, gh, gw = case
    r = np.random.default_rng([SF.SEED, 77] + list(case))
    grid = ((2 * r.integers(-12, 12, (SF.B, gh, gw, 2)) + 1) / 8.0).astype(f32)
    img, go = SF.image(case), SF.grad_output(case)
    timg = torch.from_numpy(np.transpose(img, (0, 3, 1, 2)).astype(f64)).requires_grad_(True)
    tflow = torch.from_numpy(np.transpose(grid, (0, 3, 1, 2)).astype(f64)).requires_grad_(True)
    out = R.warp_gather(timg, tflow)
    out.backward(torch.from_numpy(np.transpose(go, (0, 3, 1, 2)).astype(f64)))
    val, S = SF.forward(img, grid)
    np.testing.assert_allclose(val, out.detach().permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13 * max(1.0, float(S.max())))
    gval, gS, K = SF.image_gradient(img.shape, grid, go)
    np.testing.assert_allclose(gval, timg.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13 * max(1.0, float(gS.max())))
    assert (gS[K == 0] == 0).all() and (gval[gS == 0] == 0).all()
    ggval, ggS = SF.grid_gradient(img, grid, go)
    c = SF.cells(grid, ih, iw)
    inside = (c["xc"] > 0) & (c["xc"] < iw - 1) & (c["yc"] > 0) & (c["yc"] < ih - 1)
    if min(ih, iw) > 2:
        assert inside.sum() >= 4
    np.testing.assert_allclose(ggval[inside], tflow.grad.permute(0, 2, 3, 1).numpy()[inside], rtol=0, atol=1e-12 * max(1.0, float(ggS.max())))


@pytest.mark.parametrize("case", SAME_SIZE, ids=SF.case_id)
def test_float64_forward_is_glue_float64_warp(case):
    for field in SF.FIELDS:
        Rf = SF.reference(case, field)
        planar, flow = np.transpose(Rf["img"], (0, 3, 1, 2)), np.transpose(Rf["grid"], (0, 3, 1, 2))
        for mode, mine in (("64", Rf["fwd"][0]), ("abs", Rf["fwd"][1])):
            theirs = np.transpose(GF.warp(planar, flow, 1.0, mode), (0, 2, 3, 1))
            np.testing.assert_allclose(mine, theirs, rtol=0, atol=1e-13 * max(1.0, float(Rf["fwd"][1].max())))


# ---- the CPU oracle inside the bounds, wrong samplers outside -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SF.CASES, ids=SF.case_id)
def test_oracle_within_the_bounds(case):
    fails = []
    for field in SF.FIELDS:
        Rf = SF.reference(case, field)
        out = O.warp_bhwd(Rf["img"], Rf["grid"])
        gi, gg = O.warp_bhwd_backward(Rf["img"], Rf["grid"], Rf["grad_out"])
        val, S, K = Rf["gi"]
        for what, r, n in (("forward", SF.measure(out, *Rf["fwd"]), SF.N_FORWARD), ("grid gradient", SF.measure(gg, *Rf["gg"]), SF.n_grid(case[0])),
                           ("image gradient", SF.measure(gi, val, S * SF.n_image(K)), 1)):
            if not r <= n:
                fails.append("%s %s %s: %.3f > %d" % (SF.case_id(case), field, what, r, n))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mutate,field", [("frac", "frac"), ("frac", "edges"), ("floor-first", "edges"), ("xy", "frac"), ("xy", "edges"),
                                          ("store-yx", "frac"), ("store-yx", "whole")])
def test_a_wrong_sampler_is_outside_the_bounds(mutate, field):
    """on every case with more than one row and column: the float32 oracle held to the mutated float64 restatement misses the bounds, in the
    forward, the image gradient (store-yx: the grid gradient)"""
    for case in SF.CASES:
        C, ih, iw, gh, gw = case
        if ih == 1 or iw == 1:
            continue
        Rf = SF.reference(case, field)
        gi, gg = O.warp_bhwd_backward(Rf["img"], Rf["grid"], Rf["grad_out"])
        if mutate == "store-yx":
            assert SF.measure(gg, *SF.grid_gradient(Rf["img"], Rf["grid"], Rf["grad_out"], mutate)) > SF.n_grid(C), (case, "grid gradient")
            continue
        assert SF.measure(O.warp_bhwd(Rf["img"], Rf["grid"]), *SF.forward(Rf["img"], Rf["grid"], mutate)) > SF.N_FORWARD, (case, "forward")
        val, S, K = SF.image_gradient(Rf["img"].shape, Rf["grid"], Rf["grad_out"], mutate)
        assert SF.measure(gi, val, S * SF.n_image(K)) > 1, (case, "image gradient")
        assert SF.measure(gg, *SF.grid_gradient(Rf["img"], Rf["grid"], Rf["grad_out"], mutate)) > SF.n_grid(C), (case, "grid gradient")
