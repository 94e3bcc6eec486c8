"""CPU: the supervised objective, -optimize epe (include/b2f.h, the *_epe entries; b2f_table_loss_epe_host), without a GPU: (a) the host
entry equals the numpy restatement of the definition bit for bit, records and gradient; (b) the restatement agrees with a float64
transcription of criterions/L2Criterion.lua and train.lua:296-334 within one fp32 rounding plus a small fp64 part, and loss_summary
within the records' Q20 rounding; (c) the transcription's gradient is torch.autograd of its forward value up to the 1e-12 of
L2Criterion.lua:20,59; (d) a wrong sub-sampling stride is told from the right one; (e) malformed requests are refused with nothing
written; (f) count="batch" is "given" with the summed counts and differs from "image"; (g) the symbols, the struct and the defaults.

Largest observed fractions of the bars of (b), on the shapes and options below: gradient 0.997 of 2^-24 |v| + 2^-149 + 2^-50 |v| (the
one rounding to fp32 is half a unit in the last place, 2^-24 |v| at most, and is the whole of it); loss_summary's err 0.14 and epe 0.14
of 2^-21 per counted pixel term (both at 5 x 7, where few terms average out)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from back2future_amd import _lib, back2future, build, ops
from tests import table_loss_epe_fields as TE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["b2f_loss_epe_defaults", "b2f_table_loss_epe_host", "b2f_table_loss_epe_device", "b2f_op_table_loss_epe", "b2f_forward_loss_epe",
           "b2f_forward_loss_epe_device", "b2f_multi_forward_loss_epe"]
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


_TABLES = {}


def tables(H, W, L, past, tame=False, n=2):
    key = (H, W, L, past, tame, n)
    if key not in _TABLES:
        _TABLES[key] = TE.tables(H, W, L, past, n=n, tame=tame)
    return _TABLES[key]


def same_bits(got, want, what=""):
    """float32 arrays equal bit for bit; two NaNs in the same place count as equal"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = (g != w) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d elements differ, first at %r: got %r want %r" % (what, bad.sum(), tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def count_arg(mode, counts):
    return {TE.BATCH: "batch", TE.IMAGE: "image"}.get(mode, counts)


def host(table, gt, valid, occ, flow_scale, rescale, o, mode=TE.BATCH, counts=None):
    return ops.table_loss_epe(table, gt, valid, occ, flow_scale=flow_scale, options=TE.struct(o), count=count_arg(mode, counts), want_grad=True,
                              rescale=rescale)


def check_host(table, past, gt, valid, occ, flow_scale, rescale, o, mode=TE.BATCH, counts=None, what=""):
    rec, grad = host(table, gt, valid, occ, flow_scale, rescale, o, mode, counts)
    wrec, wgrad = TE.want(table, past, gt, valid, occ, flow_scale, rescale, o, mode, counts)
    assert rec.shape == wrec.shape and (rec == wrec).all(), "%s: records differ at %r" % (what, np.argwhere(rec != wrec)[:4].tolist())
    assert (rec[:, :, 7] == 0).all()
    for i, (g, w) in enumerate(zip(grad, wgrad)):
        same_bits(g, w, "%s tensor %d" % (what, i))
    return rec, grad


# ---- (g) symbols, struct, defaults ----

def test_symbols_struct_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "b2f.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lua = open(os.path.join(ROOT, "lua", "back2future.lua")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"B2F_API int %s\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert name + "(" in doc, name
        assert name + "(" in lua, name
    assert _lib.lib().b2f_version() >= 1012
    assert C.sizeof(_lib.LossEpeOpts) == 2 * 8 + 8 + 7 * 8           # two doubles, an int and its padding, seven doubles
    o = back2future.loss_epe_options()
    assert (o.epe, o.occ, o.size_average) == (1.0, 0.0, 0) and tuple(o.level_weights) == TE.LEVEL_WEIGHTS == back2future.LOSS_LEVEL_WEIGHTS
    s = back2future.loss_epe_options(weights={"epe": 2.0, "occ": 0.5, "level_weights": [1.0, 2.0]}, size_average=True)
    assert (s.epe, s.occ, s.size_average) == (2.0, 0.5, 1) and tuple(s.level_weights)[:3] == (1.0, 2.0, 0.02)
    for bad in ({"epe": -1.0}, {"occ": float("nan")}, {"level_weights": [float("inf")]}, {"pme": 1.0}):
        with pytest.raises(ValueError):
            back2future.loss_epe_options(weights=bad)
    assert back2future.loss_words("epe") == 8 == TE.WORDS
    assert back2future.loss_words("pme") == 16 and back2future.loss_words("finetune") == 24 and back2future.loss_words("ssim") == 32
    for src in ("back2future_amd/csrc/b2f_tableloss_epe.h", "back2future_amd/csrc/b2f_tableloss_epe.hip"):
        text = open(os.path.join(ROOT, src)).read()
        assert "train.lua:296-3" in text and "L2Criterion.lua" in text, src


# ---- (a) the host entry against the definition, bit for bit ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", TE.SHAPES)
def test_host_entry_equals_the_definition(H, W, L, past):
    """wild tables (NaN and Inf estimates) x flow_scale 20 and 10 x rescale x the four kinds of valid (1e9 and NaN under valid == 0) x
    occ 0 and 1 (unlabelled bytes 3, 7, 255) x size_average with the three count modes; an estimate equal to the ground truth at source
    pixel (0, 0) of every level"""
    table0 = tables(H, W, L, past)
    given = np.array([[3.0 + j, 5.0 + 2 * j] for j in range(L)])
    for flow_scale in (20.0, 10.0):
        for rescale in (False, True):
            for kind in TE.VALID_KINDS:
                table, gt, valid, occ = TE.ground_truth(table0, past, flow_scale, rescale, kind)
                per = 5 if past else 4
                for w_occ in (0.0, 1.0):
                    what = "%dx%d L=%d scale=%g rescale=%d valid=%s occ=%g" % (H, W, L, flow_scale, rescale, kind, w_occ)
                    rec, grad = check_host(table, past, gt, valid, occ, flow_scale, rescale, TE.opts(occ=w_occ), what=what)
                    if kind != "zero":   # e == 0 exactly: a zero in the record's sum and a gradient of exactly 0, not NaN
                        for j in range(L):
                            assert (grad[j * per][:, :, 0, 0] == 0).all() and not np.signbit(grad[j * per][:, :, 0, 0]).any(), what
                    else:
                        assert (rec[:, :, [TE.VALID, TE.EPE_Q20, TE.FLOW_NONFINITE]] == 0).all() and all((g == 0).all() for g in grad[::per]), what
                    if w_occ == 0:
                        assert (rec[:, :, 4:] == 0).all() and all(not g.view(np.uint32).any() for g in grad[per - 3::per]), what
                    for i, g in enumerate(grad):   # every tensor that is neither the future flow nor the occlusions: +0.0
                        if i % per not in (0, per - 3):
                            assert not g.view(np.uint32).any(), what
                    for mode, counts in ((TE.BATCH, None), (TE.IMAGE, None), (TE.GIVEN, given)):
                        check_host(table, past, gt, valid, occ, flow_scale, rescale, TE.opts(epe=0.75, occ=w_occ, size_average=True), mode, counts,
                                   what + " size_average mode %d" % mode)


def test_records_alone_and_gradient_alone_and_zero_weights():
    table0 = tables(48, 80, 5, True)
    table, gt, valid, occ = TE.ground_truth(table0, True, 20.0, False)
    o = TE.opts(occ=1.0)
    rec, grad = host(table, gt, valid, occ, 20.0, False, o)
    only = ops.table_loss_epe(table, gt, valid, occ, options=TE.struct(o))
    assert only.dtype == np.uint64 and (only == rec).all()
    g2 = ops.table_loss_epe(table, gt, valid, occ, options=TE.struct(o), want_loss=False, want_grad=True)
    for a, b in zip(g2, grad):
        same_bits(a, b)
    # a weight of exactly 0 switches its gradient off (+0.0, NaN estimates included); the records do not depend on the weights
    check_host(table, True, gt, valid, occ, 20.0, False, TE.opts(epe=0.0, occ=1.0), what="epe = 0")
    r0, g0 = check_host(table, True, gt, valid, occ, 20.0, False, TE.opts(epe=0.0, occ=0.0), what="both 0")
    assert all(not g.view(np.uint32).any() for g in g0) and (r0[:, :, :4] == rec[:, :, :4]).all()
    lw = (0.0, 1.0, 0.0, 2.0, 0.0, 0.0, 0.0)
    check_host(table, True, gt, valid, occ, 20.0, False, TE.opts(occ=1.0, level_weights=lw), what="level weights")


def test_a_level_without_a_valid_pixel():
    """levels 2 .. 4 have no valid source pixel: their records count nothing, and with size_average their gradient is +0.0 where the Lua
    divides by zero"""
    table0 = tables(48, 80, 5, False)
    table, gt, valid, occ = TE.ground_truth(table0, False, 20.0, True, "random", empty_level=2)
    for sa in (False, True):
        for mode in (TE.BATCH, TE.IMAGE):
            rec, grad = check_host(table, False, gt, valid, occ, 20.0, True, TE.opts(size_average=sa), mode, what="empty level")
            assert (rec[:, 2:, 1:4] == 0).all() and rec[:, :2, TE.VALID].all()
            for j in (2, 3, 4):
                assert not grad[j * 4].view(np.uint32).any()


# ---- (b) the restatement against the Lua transcription ----

@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (37, 53, 1), (16, 16, 5), (48, 80, 5)])
def test_definition_against_the_lua(H, W, L, past, record_property):
    """gradient: within 2^-24 |v| + 2^-149 + 2^-50 |v| of the transcription's float64 value v (one rounding to fp32 on store; the
    restatement forms (k d) / (e + 1e-12) where the Lua forms d / (sqrt(sum * mask) + 1e-12) * mask * k [/ N]: a few fp64 roundings);
    loss_summary: err and epe within 2^-21 per counted pixel term, times the term's factor, plus 2^-40 of the value for the fp64 sums"""
    table = tables(H, W, L, past, tame=True)
    gt, valid, occ = TE.finite_truth(table, past, 20.0)
    worst = {"grad": 0.0, "err": 0.0, "epe": 0.0}
    for flow_scale, rescale in ((20.0, False), (10.0, True)):
        for o in (TE.opts(), TE.opts(epe=0.5, occ=1.0), TE.opts(occ=2.0, size_average=True)):
            rec, grad = TE.want(table, past, gt, valid, occ, flow_scale, rescale, o)
            err, pf, po, lgrad, epe_b = TE.lua_epe(table, past, gt, valid, occ, flow_scale, rescale, o)
            for g, v in zip(grad, lgrad):
                bar = 2.0 ** -24 * np.abs(v) + 2.0 ** -149 + 2.0 ** -50 * np.abs(v)
                frac = np.abs(g.astype(np.float64) - v) / bar
                worst["grad"] = max(worst["grad"], float(frac.max()))
                assert (frac <= 1.0).all()
            s = back2future.loss_summary(rec, objective="epe", size_average=o["size_average"], flow_scale=flow_scale,
                                         weights={"epe": o["epe"], "occ": o["occ"], "level_weights": o["level_weights"]})
            N = TE.counts_of(valid, occ, rec.shape[0], H, W, L).sum(0)
            bar = 0.0
            for j in range(L):
                lw = 1.0 if o["size_average"] else o["level_weights"][j]
                nf, no = float(rec[:, j, TE.VALID].sum()), float(rec[:, j, TE.LABELLED].sum())
                bar += o["epe"] * lw * nf * 2.0 ** -21 / (N[j, 0] if o["size_average"] else 1.0)
                bar += o["occ"] * lw * no * 2.0 ** -21 / (N[j, 1] if o["size_average"] and N[j, 1] else 1.0)
            bar += 2.0 ** -40 * abs(err)
            worst["err"] = max(worst["err"], abs(s["err"] - err) / bar)
            assert abs(s["err"] - err) <= bar
            np.testing.assert_allclose(s["flow"], pf, rtol=0, atol=bar)
            np.testing.assert_allclose(s["occ"], po, rtol=0, atol=bar)
            ebar = flow_scale * 2.0 ** -21 + 2.0 ** -40 * abs(epe_b)   # the mean of VALID[0] terms of 2^-21 each, in pixels
            worst["epe"] = max(worst["epe"], abs(s["epe"] - epe_b) / ebar)
            assert abs(s["epe"] - epe_b) <= ebar
            assert s["nonfinite"] == 0
    for k, v in worst.items():
        record_property("worst_" + k, v)
    print("fractions of the bars %dx%d L=%d %s: %r" % (H, W, L, "soft" if past else "hard", worst))


# ---- (c) the transcription against torch.autograd ----

def test_lua_gradient_is_the_derivative_of_its_value():
    """at (48,80,5), every valid pixel's e in 0.05 .. 5 (and every labelled pixel's q: probabilities in 0.1 .. 0.4 are 0.1 at least from
    0, 0.5 and 1): the transcription's gradient against torch.autograd of its forward value in float64, within 64 fp64 roundings plus
    k 1e-12 / e, the effect of the 1e-12 that L2Criterion.lua:59 adds to the denominator and line 37 does not know"""
    torch = pytest.importorskip("torch")
    H, W, L, past, per = 48, 80, 5, True, 5
    table = [t.copy() for t in tables(H, W, L, past, tame=True)]
    gt, valid, occ = TE.finite_truth(table, past, 20.0)
    r = np.random.default_rng(5)
    n = table[0].shape[0]
    for j in range(L):
        h, w, s = H >> j, W >> j, 1 << j
        g = gt[:, :, ::s, ::s].astype(np.float64) / 20.0 / s
        ang, mag = r.uniform(0, 2 * np.pi, (n, 1, h, w)), r.uniform(0.06, 4.9, (n, 1, h, w))
        table[j * per] = (g + mag * np.concatenate([np.cos(ang), np.sin(ang)], 1)).astype(F32)
        table[j * per + per - 3] = r.uniform(0.1, 0.4, (n, 2, h, w)).astype(F32)
    for o in (TE.opts(occ=1.0), TE.opts(epe=0.5, occ=2.0, size_average=True)):
        err, _, _, lgrad, _ = TE.lua_epe(table, past, gt, valid, occ, 20.0, True, o)
        leaves = [torch.tensor(t.astype(np.float64), requires_grad=True) for t in table]
        total = torch.zeros((), dtype=torch.float64)
        mask = torch.tensor((valid != 0).astype(np.float64)).reshape(n, 1, H, W)
        lab = torch.tensor(occ.astype(np.int64)).reshape(n, 1, H, W)
        flow = torch.tensor(gt.astype(np.float64)) / 20.0
        for j in range(L):
            if j:
                flow, mask, lab = flow[:, :, ::2, ::2] / 2, mask[:, :, ::2, ::2], lab[:, :, ::2, ::2]
            lw = 1.0 if o["size_average"] else o["level_weights"][j]
            e = ((leaves[j * per] - flow) ** 2).sum(1, keepdim=True).sqrt()
            assert float((e.detach() * mask).max()) < 5.0 and float(e.detach()[mask > 0].min()) > 0.05
            t = torch.cat([(lab == 0) + 0.5 * (lab == 1), (lab == 2) + 0.5 * (lab == 1)], 1).double()
            m = (lab < 3).double()
            q = ((leaves[j * per + per - 3] - t) ** 2).sum(1, keepdim=True).sqrt()
            kf = o["epe"] * lw / (float(mask.sum()) if o["size_average"] else 1.0)
            ko = o["occ"] * lw / (float(m.sum()) if o["size_average"] else 1.0)
            total = total + kf * (e * mask).sum() + ko * (q * m).sum()
            for idx, k, d, mm in ((j * per, kf, e, mask), (j * per + per - 3, ko, q, m)):
                leaves[idx].bar = (k * 1e-12 / d.detach().clamp_min(1e-3) * mm).numpy()
        assert abs(float(total.detach()) - err) <= 1e-12 * abs(err)
        total.backward()
        for i, (leaf, v) in enumerate(zip(leaves, lgrad)):
            if i % per not in (0, per - 3):
                assert not v.any() and (leaf.grad is None or not leaf.grad.numpy().any())
                continue
            a = leaf.grad.numpy()
            assert np.abs(a).max() > 0
            assert (np.abs(a - v) <= 64 * 2.0 ** -53 * np.abs(a) + leaf.bar).all(), i


# ---- (d) the sub-sampling ----

def test_a_wrong_stride_fails():
    """ground truth whose value is its own coordinate, and estimates that hold (x << j, y << j) over flow_scale: exact zeros on every
    level when level j reads (y << j, x << j); the same field shifted by one source pixel gives a whole pixel of error everywhere"""
    H, W, L, n, scale = 48, 80, 5, 2, 16.0
    ys, xs = np.mgrid[0:H, 0:W]
    gt = np.broadcast_to(np.stack([xs, ys]).astype(F32)[None], (n, 2, H, W)).copy()
    table = []
    for j in range(L):
        y, x = np.mgrid[0:H >> j, 0:W >> j]
        f = np.broadcast_to((np.stack([x << j, y << j]) / scale).astype(F32)[None], (n, 2, H >> j, W >> j)).copy()
        table += [f, np.zeros_like(f), np.zeros((n, 3, H >> j, W >> j), F32), np.zeros((n, 3, H >> j, W >> j), F32)]
    rec, grad = ops.table_loss_epe(table, gt, flow_scale=scale, want_grad=True)
    for j in range(L):
        assert (rec[:, j, TE.VALID] == (H >> j) * (W >> j)).all() and (rec[:, j, TE.EPE_Q20] == 0).all() and not grad[4 * j].any()
    for axis in (2, 3):
        shifted = np.roll(gt, 1, axis=axis)
        rec = ops.table_loss_epe(table, shifted, flow_scale=scale)
        for j in range(L):
            assert (rec[:, j, TE.EPE_Q20] >= ((H >> j) * (W >> j) << 20) // int(scale)).all(), (axis, j)
    # with rescale the same estimates are wrong from level 1 on, and right again once they are halved per level
    rec = ops.table_loss_epe(table, gt, flow_scale=scale, rescale=True)
    assert (rec[:, 0, TE.EPE_Q20] == 0).all() and (rec[:, 1:, TE.EPE_Q20] > 0).all()
    halved = [t / F32(1 << (i // 4)) if i % 4 == 0 else t for i, t in enumerate(table)]
    assert (ops.table_loss_epe(halved, gt, flow_scale=scale, rescale=True)[:, :, TE.EPE_Q20] == 0).all()


# ---- (e) refusals ----

def test_refusals_write_nothing():
    H, W, L, n, per = 16, 16, 2, 2, 4
    table = tables(H, W, L, False)
    table, gt, valid, occ = TE.ground_truth(table, False, 20.0, False)
    lib = _lib.lib()
    fill = 0x5A5A5A5A5A5A5A5A
    loss = np.full((n, L, TE.WORDS), fill, np.uint64)
    grad = [np.full(t.shape, F32(7.5), F32) for t in table]
    ptrs = (_lib.c_float_p * len(table))(*[_lib.fptr(t) for t in table])
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    good = dict(table=ptrs, n_outs=len(table), n=n, H=H, W=W, past=0, gt=_lib.fptr(gt), valid=u8(valid), occ=u8(occ), scale=20.0, rescale=0,
                opts=None, mode=TE.BATCH, counts=None, loss=lp, grad=gp)
    order = ("table", "n_outs", "n", "H", "W", "past", "gt", "valid", "occ", "scale", "rescale", "opts", "mode", "counts", "loss", "grad")

    def call(**kw):
        a = dict(good, **kw)
        return lib.b2f_table_loss_epe_host(*[a[k] for k in order])

    assert call() == 0 and loss[0, 0, 0] == H * W
    loss[:] = fill
    for g in grad:
        g[:] = F32(7.5)

    def opts(**kw):
        o = back2future.loss_epe_options()
        for k, v in kw.items():
            if k == "lw":
                o.level_weights[1] = v
            else:
                setattr(o, k, v)
        return C.byref(o)

    counts = lambda v: np.array(v, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    aliased = (_lib.c_float_p * len(grad))(*([_lib.fptr(table[0])] + [_lib.fptr(g) for g in grad[1:]]))
    twice = (_lib.c_float_p * len(grad))(*([_lib.fptr(grad[1])] + [_lib.fptr(g) for g in grad[1:]]))
    on_gt = (_lib.c_float_p * len(grad))(*([_lib.fptr(gt)] + [_lib.fptr(g) for g in grad[1:]]))
    holed = (_lib.c_float_p * len(grad))(*([None] + [_lib.fptr(g) for g in grad[1:]]))
    bad = [("null gt_flow", dict(gt=None)), ("null table", dict(table=None)), ("loss and grad", dict(loss=None, grad=None)),
           ("negative epe", dict(opts=opts(epe=-1.0))), ("nan epe", dict(opts=opts(epe=float("nan")))), ("inf occ", dict(opts=opts(occ=float("inf")))),
           ("negative occ", dict(opts=opts(occ=-0.5))), ("negative level weight", dict(opts=opts(lw=-1.0))), ("nan level weight", dict(opts=opts(lw=float("nan")))),
           ("occ without gt_occ", dict(opts=opts(occ=1.0), occ=None)), ("count_mode 3", dict(mode=3)), ("count_mode -1", dict(mode=-1)),
           ("given without counts", dict(mode=TE.GIVEN)), ("negative count", dict(mode=TE.GIVEN, counts=counts([[1, 1], [-1, 1]]))),
           ("nan count", dict(mode=TE.GIVEN, counts=counts([[1, float("nan")], [1, 1]]))), ("n_outs 3", dict(n_outs=3)), ("n 0", dict(n=0)),
           ("H not a multiple", dict(H=15)), ("flow_scale 0", dict(scale=0.0)), ("flow_scale nan", dict(scale=float("nan"))),
           ("2^28 pixels", dict(H=1 << 14, W=1 << 14)), ("grad aliases the table", dict(grad=aliased)), ("grad aliases itself", dict(grad=twice)),
           ("grad aliases gt_flow", dict(grad=on_gt)), ("null tensor in grad", dict(grad=holed)),
           ("loss aliases gt_flow", dict(loss=C.cast(_lib.fptr(gt), C.POINTER(C.c_ulonglong))))]
    for what, kw in bad:
        assert call(**kw) != 0, what
        assert lib.b2f_last_error(), what
        assert (loss == fill).all() and all((g == F32(7.5)).all() for g in grad), what + ": something was written"
    # the wrappers refuse before the library is called
    for kw in (dict(count="all"), dict(count=np.ones((3, 2))), dict(options=back2future.loss_grad_options()), dict(want_loss=False)):
        with pytest.raises(ValueError):
            ops.table_loss_epe(table, gt, valid, occ, **kw)
    with pytest.raises(ValueError):
        ops.table_loss_epe(table, gt[:, :1], valid, occ)
    with pytest.raises(ValueError):
        ops.table_loss_epe(table, gt, valid.astype(np.float32), occ)
    with pytest.raises(_lib.B2FError, match="occ > 0 needs gt_occ"):
        ops.table_loss_epe(table, gt, valid, None, options=back2future.loss_epe_options(weights={"occ": 1.0}))
    with pytest.raises(ValueError):
        ops.table_loss(table, np.zeros((n, 3, H, W), F32), objective="epe")
    with pytest.raises(ValueError):
        back2future.loss_summary(np.zeros((n, L, 16), np.uint64), objective="epe")
    with pytest.raises(ValueError):
        back2future.loss_summary(np.zeros((n, L, 8), np.uint64), objective="epe", like="train")


# ---- (f) the counts ----

def test_batch_count_is_given_with_the_summed_counts():
    H, W, L, n, past, per = 16, 16, 5, 3, True, 5
    table = tables(H, W, L, past, n=n)
    table, gt, valid, occ = TE.ground_truth(table, past, 20.0, False, "random", seed=3)
    o = TE.opts(occ=1.0, size_average=True)
    own = TE.counts_of(valid, occ, n, H, W, L)
    assert len({tuple(own[b, 0]) for b in range(n)}) == n                  # the images differ in their counts
    _, batch = check_host(table, past, gt, valid, occ, 20.0, False, o, TE.BATCH)
    _, given = check_host(table, past, gt, valid, occ, 20.0, False, o, TE.GIVEN, own.sum(0))
    _, image = check_host(table, past, gt, valid, occ, 20.0, False, o, TE.IMAGE)
    for i in range(0, len(table), per):
        for t in (i, i + per - 3):
            same_bits(batch[t], given[t])
        if own[:, i // per, 0].min() > 0 and (H >> (i // per)) > 1:
            assert (batch[i] != image[i]).any()
    # one image at a time with its own counts is count="image" of the batch: a cut changes nothing there
    for b in range(n):
        _, one = host([t[b:b + 1] for t in table], gt[b:b + 1], valid[b:b + 1], occ[b:b + 1], 20.0, False, o, TE.BATCH)
        for i in range(len(table)):
            same_bits(one[i], image[i][b:b + 1])
    # loss_summary: the batch's counts from the records, and per image
    rec = ops.table_loss_epe(table, gt, valid, occ, options=TE.struct(o))
    s_b = back2future.loss_summary(rec, objective="epe", size_average=True, weights={"occ": 1.0})
    s_g = back2future.loss_summary(rec, objective="epe", size_average=True, weights={"occ": 1.0}, count=own.sum(0))
    s_i = back2future.loss_summary(rec, objective="epe", size_average=True, weights={"occ": 1.0}, count="image")
    assert s_b["nonfinite"] > 0                                              # wild tables: N_j counts the valid pixels, finite or not
    np.testing.assert_allclose(s_b["flow"], s_g["flow"], rtol=1e-15)
    np.testing.assert_allclose(s_b["occ"], s_g["occ"], rtol=1e-15)
    assert not np.allclose(s_b["flow"], s_i["flow"])
