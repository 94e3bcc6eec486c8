"""GPU: the supervised objective, -optimize epe (include/b2f.h, the *_epe entries; train.lua:296-334 with criterions/L2Criterion.lua) on
the device.  b2f_op_table_loss_epe and b2f_table_loss_epe_device against the host entry b2f_table_loss_epe_host (which
tests/test_table_loss_epe_cpu.py holds against a numpy restatement of the definition): records equal word for word and every gradient
element bit for bit -- the per-pixel arithmetic is fp64 without contraction, + - * / and sqrt only, the records are integer sums and an
element is rounded to fp32 once, so no tolerance is involved anywhere.  Everything above the kernel is defined from it:
Model.forwardLoss / forwardLossGrad with objective="epe" give ops.table_loss_epe of the table Model.forward returns, however the request is
cut or sharded."""
import contextlib

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import table_loss_epe_fields as TE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# The launch caps the grid of one image at 1024 blocks of 256 threads, a thread per group of four pixels of a row: 262144 groups.
# 481 rows of 545 groups (2177 columns, an odd width: scalar loads and stores) are 262145 groups: the first thread alone takes a
# second one.
WRAP = (481, 2177, 1)
GUARD = 4096


@pytest.fixture(scope="module")
def models():
    m = {False: back2future.Model("random:hard:5:2.0"), True: back2future.Model("random:soft:5:2.0")}
    yield m
    for v in m.values():
        v.close()


def _same(got, want, what):
    """lists of float32 arrays equal bit for bit; two NaNs in the same place count as equal"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (what, i, g.shape, w.shape)
        bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: tensor %d: %d elements differ, first at %r: %r, expected %r" % (what, i, bad.sum(), at, g[at], w[at]))


def _both(m, table, gt, valid, occ, o, what, flow_scale=20.0, count="batch"):
    """records and gradient from one call, the records alone and the gradient alone: the op entry against the host entry"""
    s = TE.struct(o)
    kw = dict(flow_scale=flow_scale, options=s, count=count)
    rec, grad = ops.table_loss_epe(table, gt, valid, occ, want_grad=True, model=m, **kw)
    wrec, wgrad = ops.table_loss_epe(table, gt, valid, occ, want_grad=True, **kw)
    assert rec.dtype == np.uint64 and rec.shape == wrec.shape and np.array_equal(rec, wrec), (what, np.argwhere(rec != wrec)[:4].tolist())
    _same(grad, wgrad, what)
    return rec, grad


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L", TE.SHAPES)
def test_op_table_loss_epe_matches_the_host_entry(models, H, W, L, past):
    """The sizes of the CPU test: one pixel, one row, one column, partial groups, odd widths (rows and planes start at addresses that
    are no multiple of 16 resp. 4 bytes: scalar loads and stores), (16,16,5) down to 1 x 1, (48,80,5) with strides 1 .. 16 into the
    ground truth.  Wild tables (NaN and Inf estimates), the four kinds of valid with 1e9 and NaN under valid == 0, unlabelled bytes,
    flow_scale 20 and 10, occ 0 and 1 (the four kernel instances), size_average with the three count modes, records alone."""
    m = models[past]
    table0 = TE.tables(H, W, L, past)
    given = np.array([[3.0 + j, 5.0 + 2 * j] for j in range(L)])
    what = "%dx%d L=%d" % (H, W, L)
    for kind in TE.VALID_KINDS:
        flow_scale = 10.0 if kind == "one" else 20.0
        table, gt, valid, occ = TE.ground_truth(table0, past, flow_scale, False, kind)
        for w_occ in (0.0, 1.0):
            w = "%s valid=%s occ=%g" % (what, kind, w_occ)
            rec, _ = _both(m, table, gt, valid, occ, TE.opts(occ=w_occ), w, flow_scale)
            only = ops.table_loss_epe(table, gt, valid, occ, flow_scale=flow_scale, options=TE.struct(TE.opts(occ=w_occ)), model=m)
            assert np.array_equal(only, rec), w + " records alone"
            for count in ("batch", "image", given):
                _both(m, table, gt, valid, occ, TE.opts(epe=0.75, occ=w_occ, size_average=True), w + " size_average", flow_scale, count)
    table, gt, valid, occ = TE.ground_truth(table0, past, 20.0, False, "random")
    _both(m, table, gt, valid, occ, TE.opts(epe=0.0, occ=1.0, level_weights=(1.0, 0.0, 2.0, 0.0, 1.0, 0.0, 0.0)), what + " zero weights")


def test_one_group_more_than_the_capped_grid_has_threads(models):
    H, W, L = WRAP
    table = TE.tables(H, W, L, False, n=1)
    table, gt, valid, occ = TE.ground_truth(table, False, 20.0, False, "random")
    rec, _ = _both(models[False], table, gt, valid, occ, TE.opts(occ=1.0, size_average=True), "%dx%d" % (H, W))
    assert rec[0, 0, TE.PIXELS] == H * W


def test_rescale_flow_comes_from_the_context():
    """a context made with rescale_flow=1 divides the ground truth by 2^j as train.lua:300-302 does: the host entry with rescale=True"""
    m = back2future.Model("random:soft:3:2.0", graph="win=5,levels=4,skip=2,rescale_flow=1")
    try:
        H, W, L = 32, 48, 2
        table = TE.tables(H, W, L, True)
        table, gt, valid, occ = TE.ground_truth(table, True, 20.0, True, "random")
        s = TE.struct(TE.opts(occ=1.0, size_average=True))
        rec, grad = ops.table_loss_epe(table, gt, valid, occ, options=s, want_grad=True, model=m)
        wrec, wgrad = ops.table_loss_epe(table, gt, valid, occ, options=s, want_grad=True, rescale=True)
        assert np.array_equal(rec, wrec) and not np.array_equal(rec, ops.table_loss_epe(table, gt, valid, occ, options=s))
        _same(grad, wgrad, "rescale_flow=1")
    finally:
        m.close()


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_device_entry_on_a_side_stream_right_behind_the_uploads(models, past):
    """... and the inputs are unchanged after the call; aliased, misaligned and host pointers, bad options and counts are refused with
    nothing written and nothing launched."""
    H, W, L, n = 48, 80, 3, 2
    m = models[past]
    table = TE.tables(H, W, L, past, n=n, seed=3)
    table, gt, valid, occ = TE.ground_truth(table, past, 20.0, False, "random")
    opt = back2future.loss_epe_options(weights={"occ": 1.0}, size_average=True)
    stream = torch.cuda.Stream()
    grad = [torch.full(t.shape, 7.0, dtype=torch.float32, device="cuda") for t in table]
    loss = torch.full((n, L, TE.WORDS), 7, dtype=torch.int64, device="cuda")
    host_in = table + [gt, valid, occ]
    pinned = [torch.from_numpy(t).pin_memory() for t in host_in]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dev = [t.to("cuda", non_blocking=True) for t in pinned]
        tp, (gtp, vp, op_) = [d.data_ptr() for d in dev[:-3]], [d.data_ptr() for d in dev[-3:]]
        gp = [g.data_ptr() for g in grad]
        m.tableLossGradDevice(tp, n, H, W, None, gp, options=opt, stream=stream.cuda_stream, objective="epe", gt_flow=gtp, valid=vp, gt_occ=op_,
                              count="image", d_loss=loss.data_ptr())
    stream.synchronize()
    wrec, wgrad = ops.table_loss_epe(table, gt, valid, occ, options=opt, count="image", want_grad=True)
    _same([g.cpu().numpy() for g in grad], wgrad, "device entry")
    assert np.array_equal(loss.cpu().numpy().view(np.uint64), wrec)
    loss.fill_(7)
    torch.cuda.synchronize()
    m.tableLossDevice(tp, n, H, W, None, loss.data_ptr(), objective="epe", gt_flow=gtp, valid=vp, gt_occ=op_, options=opt)
    m.synchronize()
    assert np.array_equal(loss.cpu().numpy().view(np.uint64), wrec)
    for d, t in zip(dev, host_in):
        assert np.array_equal(d.cpu().numpy().view(np.uint8), t.view(np.uint8))          # the inputs are read only
    for g in grad:
        g.fill_(7.0)
    loss.fill_(7)
    torch.cuda.synchronize()
    m.profile_reset()
    m.set_option("profile", 1)
    call = lambda **kw: m.tableLossGradDevice(kw.pop("tp", tp), n, H, W, None, kw.pop("gp", gp), objective="epe",
                                              **dict(dict(options=opt, gt_flow=gtp, valid=vp, gt_occ=op_, d_loss=loss.data_ptr()), **kw))
    try:
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: the gradient table must not alias the table"):
            call(gp=[tp[0]] + gp[1:])
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: the gradient table must not alias the ground truth"):
            call(gp=gp[:-1] + [gtp])
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: the gradient table must not alias loss"):
            call(gp=[loss.data_ptr()] + gp[1:])
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: loss must not alias an input"):
            call(d_loss=gtp)
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: device buffers must be 16-byte aligned"):
            call(gp=[gp[0] + 4] + gp[1:])
        with pytest.raises(_lib.B2FError, match="host memory"):
            call(gt_flow=gt.ctypes.data & ~15)
        with pytest.raises(_lib.B2FError, match="n_outs"):
            call(tp=tp[:7], gp=gp[:7])
        with pytest.raises(_lib.B2FError, match="occ > 0 needs gt_occ"):
            call(gt_occ=None)
        with pytest.raises(ValueError, match="needs gt_flow"):
            call(gt_flow=None)
        with pytest.raises(_lib.B2FError, match="counts must be finite and >= 0"):
            call(count=np.array([[1.0, 1.0], [1.0, -2.0], [1.0, 1.0]]))
        bad = back2future.loss_epe_options()
        bad.epe = float("nan")
        with pytest.raises(_lib.B2FError, match="finite and >= 0"):
            call(options=bad)
        ptrs = (_lib.C.c_void_p * len(tp))(*tp)
        gptrs = (_lib.C.c_void_p * len(gp))(*gp)
        with pytest.raises(_lib.B2FError, match="count_mode"):
            _lib.check(_lib.lib().b2f_table_loss_epe_device(m._h, ptrs, len(tp), n, H, W, gtp, vp, op_, 20.0, None, 5, None, loss.data_ptr(), gptrs, None))
        with pytest.raises(_lib.B2FError, match="both null"):
            _lib.check(_lib.lib().b2f_table_loss_epe_device(m._h, ptrs, len(tp), n, H, W, gtp, vp, op_, 20.0, None, 0, None, None, None, None))
        torch.cuda.synchronize()
        assert not [k for k, (ms, cnt) in m.profile_read().items() if cnt > 0 and k.startswith("table_loss")]      # a refused call launches nothing
    finally:
        m.set_option("profile", 0)
    assert all((g.cpu().numpy() == 7.0).all() for g in grad) and (loss.cpu().numpy() == 7).all()        # and writes nothing
    # a call that runs is the row table_loss_epe
    m.set_option("profile", 1)
    try:
        call()
        m.synchronize()
        assert [k for k, (ms, cnt) in m.profile_read().items() if cnt > 0 and k.startswith("table_loss")] == ["table_loss_epe"]
    finally:
        m.set_option("profile", 0)
    _same([g.cpu().numpy() for g in grad], ops.table_loss_epe(table, gt, valid, occ, options=opt, want_loss=False, want_grad=True), "after the refusals")


def test_two_frame_contexts_are_refused():
    m = back2future.Model("random:hard:3:2.0", graph="two_frame=1")
    try:
        table = TE.tables(16, 16, 1, False)
        gt = np.zeros((2, 2, 16, 16), np.float32)
        with pytest.raises(_lib.B2FError, match="b2f_table_loss_epe_device: a two_frame model"):
            ops.table_loss_epe(table, gt, model=m)
    finally:
        m.close()


def test_the_op_entry_under_guards():
    """arena_guard = 4096 floats and arena_fill = 1: the op entry's staging buffers -- table, ground truth, byte planes, records, gradient
    -- are guarded and start as a NaN pattern; words and bits are those of the host entry and b2f_arena_check finds every guard word in
    place."""
    g = back2future.Model("random:soft:5:2.0")
    try:
        g.set_option("arena_guard", GUARD)
        g.set_option("arena_fill", 1)
        for H, W, L in ((37, 53, 1), (48, 80, 5)):
            table = TE.tables(H, W, L, True)
            table, gt, valid, occ = TE.ground_truth(table, True, 20.0, False, "random")
            for count in ("batch", "image"):
                _both(g, table, gt, valid, occ, TE.opts(occ=1.0, size_average=True), "guarded op entry %dx%d %s" % (H, W, count), count=count)
                assert g.arena_check() == 0
            _both(g, table, gt, None, None, TE.opts(), "guarded op entry without the byte planes")
            assert g.arena_check() == 0
    finally:
        g.close()


# ---- behind model:forward ----

MEAN = np.array([0.485, 0.456, 0.406] * 3, np.float32).reshape(1, 9, 1, 1)
STD = np.array([0.229, 0.224, 0.225] * 3, np.float32).reshape(1, 9, 1, 1)


def _input(seed, n, H, W):
    r = np.random.default_rng(seed)
    return ((r.random((n, 9, H, W), dtype=np.float32) + (-MEAN)) / STD).astype(np.float32)


def _truth(seed, n, H, W):
    """ground truth for a forward pass: flows of a few pixels, 1e9 and NaN under valid == 0, labels 0 / 1 / 2 and unlabelled bytes"""
    r = np.random.default_rng(seed)
    gt = (r.standard_normal((n, 2, H, W)) * 3.0).astype(np.float32)
    valid = (r.random((n, H, W)) < 0.6 + 0.1 * np.arange(n)[:, None, None]).astype(np.uint8)
    gt[:, 0][valid == 0] = np.float32(1e9)
    gt[:, 1][valid == 0] = np.float32(np.nan)
    occ = r.choice(np.array([0, 1, 2, 3, 255], np.uint8), size=(n, H, W))
    return gt, valid, np.ascontiguousarray(occ)


def _rec_same(a, b, what):
    assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_forward_loss_grad_is_the_table_loss_epe_of_forward(models, past):
    """3 x 128 x 192: records and gradient of the table that never left the GPU are those of the downloaded one, whole and in three
    sub-batches -- with size_average and count="batch", the case a cut could break: the counts are taken over the whole request first
    --; want_table returns Model.forward's bits; the device entry leaves the same in the caller's tensors and refuses the batch's counts
    when it would be cut."""
    m = models[past]
    n, H, W = 3, 128, 192
    x = _input(61 + past, n, H, W)
    gt, valid, occ = _truth(7 + past, n, H, W)
    table = m.forward(x)
    sa = back2future.loss_epe_options(weights={"epe": 0.5, "occ": 1.0}, size_average=True)
    plain = back2future.loss_epe_options(weights={"occ": 0.25})
    want = {}
    for key, opt, count in (("sa batch", sa, "batch"), ("sa image", sa, "image"), ("plain", plain, "batch")):
        want[key] = ops.table_loss_epe(table, gt, valid, occ, options=opt, count=count, want_grad=True)
    rec_w, grad_w = want["sa batch"]
    assert rec_w.shape == (n, 5, TE.WORDS) and rec_w[:, :, TE.VALID].all() and rec_w[:, :, TE.LABELLED].all()
    assert all(np.isfinite(g).all() for g in grad_w) and all(float(np.abs(grad_w[i]).max()) > 0 for i in range(0, len(table), 5 if past else 4))
    assert any(not np.array_equal(a, b) for a, b in zip(grad_w, want["sa image"][1]))        # the images differ in their counts
    kw = dict(objective="epe", gt_flow=gt, valid=valid, gt_occ=occ)
    for sub in (None, H * W):
        with (m.options(host_subbatch_pixels=sub) if sub else contextlib.nullcontext()):
            what = "three sub-batches" if sub else "whole"
            for key, opt, count in (("sa batch", sa, "batch"), ("sa image", sa, "image"), ("plain", plain, "batch")):
                grad, rec = m.forwardLossGrad(x, options=opt, count=count, **kw)
                _same(grad, want[key][1], what + " " + key)
                _rec_same(rec, want[key][0], what + " " + key)
            _same(m.forwardLossGrad(x, options=sa, want_loss=False, **kw), grad_w, what + " without the records")
            _rec_same(m.forwardLoss(x, options=sa, **kw), rec_w, what + " forwardLoss")
            grad, rec, tab = m.forwardLossGrad(x, options=sa, want_table=True, **kw)
            _same(grad, grad_w, what + " with the table")
            _same(tab, table, what + " table")
            rec, tab = m.forwardLoss(x, options=sa, want_table=True, **kw)
            _rec_same(rec, rec_w, what + " forwardLoss with the table")
            _same(tab, table, what + " forwardLoss table")
    # without valid and gt_occ
    rec0, grad0 = ops.table_loss_epe(table, gt * 0, want_grad=True)
    grad, rec = m.forwardLossGrad(x, objective="epe", gt_flow=gt * 0)
    _same(grad, grad0, "no byte planes")
    _rec_same(rec, rec0, "no byte planes")
    # the device entries on a side stream, behind the uploads
    stream = torch.cuda.Stream()
    pinned = [torch.from_numpy(a).pin_memory() for a in (x, gt, valid, occ)]
    for sub, count in ((None, "batch"), (H * W, "image")):
        dg = [torch.full(t.shape, 7.0, dtype=torch.float32, device="cuda") for t in table]
        loss = torch.full((n, 5, TE.WORDS), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with (m.options(host_subbatch_pixels=sub) if sub else contextlib.nullcontext()):
            with torch.cuda.stream(stream):
                dx, dgt, dv, do = [t.to("cuda", non_blocking=True) for t in pinned]
                m.forwardLossGradDevice(dx.data_ptr(), n, H, W, [g.data_ptr() for g in dg], d_loss=loss.data_ptr(), options=sa, stream=stream.cuda_stream,
                                        objective="epe", gt_flow=dgt.data_ptr(), valid=dv.data_ptr(), gt_occ=do.data_ptr(), count=count)
            stream.synchronize()
            key = "sa " + count
            _same([g.cpu().numpy() for g in dg], want[key][1], "forwardLossGradDevice " + key)
            _rec_same(loss.cpu().numpy().view(np.uint64), want[key][0], "forwardLossGradDevice " + key)
            loss.fill_(7)
            torch.cuda.synchronize()
            m.forwardLossDevice(dx.data_ptr(), n, H, W, loss.data_ptr(), objective="epe", gt_flow=dgt.data_ptr(), valid=dv.data_ptr(), gt_occ=do.data_ptr(),
                                options=sa)
            m.synchronize()
            _rec_same(loss.cpu().numpy().view(np.uint64), rec_w, "forwardLossDevice")
            if sub:
                for g in dg:
                    g.fill_(7.0)
                torch.cuda.synchronize()
                with pytest.raises(_lib.B2FError, match="b2f_forward_loss_epe_device: B2F_EPE_COUNT_BATCH needs the request in one sub-batch"):
                    m.forwardLossGradDevice(dx.data_ptr(), n, H, W, [g.data_ptr() for g in dg], options=sa, objective="epe", gt_flow=dgt.data_ptr(),
                                            valid=dv.data_ptr(), gt_occ=do.data_ptr(), count="batch")
                torch.cuda.synchronize()
                assert all((g.cpu().numpy() == 7.0).all() for g in dg)
    with pytest.raises(_lib.B2FError, match="b2f_forward_loss_epe: occ > 0 needs gt_occ"):
        m.forwardLossGrad(x, options=sa, objective="epe", gt_flow=gt, valid=valid)
    with pytest.raises(ValueError, match="needs gt_flow"):
        m.forwardLossGrad(x, options=sa, objective="epe")
    with pytest.raises(_lib.B2FError, match="b2f_forward_loss_epe_device: in_kind must be B2F_IN_NORMALIZED"):
        ptrs = (_lib.C.c_void_p * len(dg))(*[g.data_ptr() for g in dg])
        _lib.check(_lib.lib().b2f_forward_loss_epe_device(m._h, dx.data_ptr(), back2future.IN_UNIT, n, H, W, dgt.data_ptr(), None, None, 20.0, None, 0, None,
                                                          None, ptrs, len(dg), None))
    # calls that do not name the objective behave as before
    g16, r16 = m.forwardLossGrad(x)
    assert r16.shape == (n, 5, 16) and np.array_equal(r16, m.forwardLoss(x))


def test_multi_forward_loss_epe_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) on two replicas of one GPU give one context's bits with count="image"; the batch's counts are refused"""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        n, H, W = 3, 128, 192
        x = _input(21, n, H, W)
        gt, valid, occ = _truth(3, n, H, W)
        opt = back2future.loss_epe_options(weights={"occ": 1.0}, size_average=True)
        kw = dict(objective="epe", gt_flow=gt, valid=valid, gt_occ=occ, options=opt)
        want, rec_want = ref.forwardLossGrad(x, count="image", **kw)
        assert len(want) == 25 and rec_want.shape == (n, 5, TE.WORDS) and float(np.abs(want[0]).max()) > 0
        grad, rec = mm.forwardLossGrad(x, **kw)
        _same(grad, want, "two replicas")
        _rec_same(rec, rec_want, "two replicas")
        _same(mm.forwardLossGrad(x, want_loss=False, **kw), want, "two replicas without the records")
        _rec_same(mm.forwardLoss(x, **kw), rec_want, "two replicas forwardLoss")
        with pytest.raises(ValueError, match="count must be 'image'"):
            mm.forwardLossGrad(x, count="batch", **kw)
        gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
        with pytest.raises(_lib.B2FError, match="b2f_multi_forward_loss_epe: B2F_EPE_COUNT_BATCH is not served over several GPUs"):
            _lib.check(_lib.lib().b2f_multi_forward_loss_epe(mm._h, _lib.fptr(x), n, H, W, _lib.fptr(gt), None, None, 20.0, None, 0, None, None, gp, len(grad)))
    finally:
        mm.close()
        ref.close()


def test_a_context_made_with_options_and_a_two_frame_one_behind_forward():
    """win=5,levels=4,skip=2: a table of two levels from the generic executor; two_frame is refused with nothing written."""
    opt = back2future.loss_epe_options(weights={"occ": 1.0}, size_average=True)
    m = back2future.Model("random:soft:3:2.0", graph="win=5,levels=4,skip=2")
    try:
        x = _input(31, 2, 32, 48)
        gt, valid, occ = _truth(5, 2, 32, 48)
        table = m.forward(x)
        assert len(table) == 10
        rec_w, grad_w = ops.table_loss_epe(table, gt, valid, occ, options=opt, want_grad=True)
        grad, rec = m.forwardLossGrad(x, options=opt, objective="epe", gt_flow=gt, valid=valid, gt_occ=occ)
        _same(grad, grad_w, "win=5,levels=4,skip=2")
        _rec_same(rec, rec_w, "win=5,levels=4,skip=2")
        r2, g2 = ops.table_loss_epe(table, gt, valid, occ, options=opt, want_grad=True, model=m)
        _same(g2, grad_w, "op on the generic table")
        _rec_same(r2, rec_w, "op on the generic table")
    finally:
        m.close()
    m = back2future.Model("random:hard:3:2.0", graph="two_frame=1")
    try:
        x = _input(32, 1, 64, 64)
        gt = np.zeros((1, 2, 64, 64), np.float32)
        shapes = m.output_shapes(64, 64)
        host = [np.full((1,) + s, 7.0, np.float32) for s in shapes]
        gp = (_lib.c_float_p * len(host))(*[_lib.fptr(g) for g in host])
        with pytest.raises(_lib.B2FError, match="b2f_forward_loss_epe: a two_frame model"):
            _lib.check(_lib.lib().b2f_forward_loss_epe(m._h, _lib.fptr(x), 1, 64, 64, _lib.fptr(gt), None, None, 20.0, None, 0, None, None, gp, len(host), None))
        assert all((g == 7.0).all() for g in host)
    finally:
        m.close()


def test_validate_example_prints_the_summary(tmp_path):
    """examples/validate.py --objective epe --gt GT_DIR --occ-weight 0.5 --size-average --grad on four 70 x 130 PNGs (cropped to
    64 x 128) with .flo, _valid.png and _occ.png files: value for value back2future.loss_summary of the records of
    Model.forwardLossGrad(objective="epe"), then the norms of its gradient."""
    import os
    import subprocess
    import sys
    from PIL import Image
    from back2future_amd import flow_io
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = np.random.default_rng(15)
    names = ["f%02d" % t for t in range(4)]
    frames = r.integers(0, 256, (4, 70, 130, 3), dtype=np.uint8)
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    gt = (r.standard_normal((2, 2, 70, 130)) * 3.0).astype(np.float32)
    valid = (r.random((2, 70, 130)) < 0.7).astype(np.uint8)
    grey = r.choice(np.array([0, 127, 128, 255, 60], np.uint8), size=(2, 70, 130))
    for nm, f in zip(names, frames):
        Image.fromarray(f).save(str(tmp_path / (nm + ".png")))
    for i, nm in enumerate(names[1:-1]):
        flow_io.writeFLO(str(gt_dir / (nm + ".flo")), gt[i])
        Image.fromarray(valid[i] * np.uint8(255)).save(str(gt_dir / (nm + "_valid.png")))
        Image.fromarray(grey[i]).save(str(gt_dir / (nm + "_occ.png")))
    lut = np.full(256, 255, np.uint8)
    lut[0], lut[127], lut[128], lut[255] = 0, 1, 1, 2
    norm = [back2future.normalize(np.ascontiguousarray(f[:64, :128].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)) for f in frames]
    x = np.stack([np.concatenate(norm[i:i + 3], axis=0) for i in range(2)])
    opt = back2future.loss_epe_options(weights={"occ": 0.5}, size_average=True)
    m = back2future.Model("random:soft:5:2.0")
    try:
        grad, rec = m.forwardLossGrad(x, options=opt, objective="epe", gt_flow=np.ascontiguousarray(gt[:, :, :64, :128]), valid=valid[:, :64, :128],
                                      gt_occ=lut[grey[:, :64, :128]], count="image")
    finally:
        m.close()
    script = os.path.join(root, "examples", "validate.py")
    p = subprocess.run([sys.executable, script, str(tmp_path), "random:soft:5:2.0", "--objective", "epe", "--gt", str(gt_dir), "--occ-weight", "0.5",
                        "--size-average", "--grad"], check=True, timeout=300, capture_output=True)
    lines = p.stdout.decode().splitlines()
    s = back2future.loss_summary(rec, objective="epe", size_average=True, weights={"occ": 0.5}, count="image")
    assert s["err"] > 0 and s["occ"].all() and s["epe"] > 0
    want = ["err %r" % s["err"]] + ["flow %d %r" % (j, float(v)) for j, v in enumerate(s["flow"])] + ["occ %d %r" % (j, float(v)) for j, v in enumerate(s["occ"])]
    want += ["epe %r" % s["epe"], "nonfinite %d" % s["nonfinite"]]
    want += ["grad %d %s %r %r" % (i // 5, ("f", "p", "o", "iw1", "iw3")[i % 5], float(np.sqrt(float((g.astype(np.float64) ** 2).sum()))), float(np.abs(g).max()))
             for i, g in enumerate(grad)]
    assert lines == want and len(want) == 1 + 5 + 5 + 2 + 25
    bad = subprocess.run([sys.executable, script, str(tmp_path), "random:soft:5:2.0", "--objective", "epe"], capture_output=True, timeout=300)
    assert bad.returncode != 0 and b"--gt GT_DIR" in bad.stderr
