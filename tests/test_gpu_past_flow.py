"""GPU: the Soft models' past flow (skip_ubfs[3], models/pwc.lua:328-385) as an output of the pruned forward pass and of the
computeFlow boundary, and motion compensation with it (pwc.lua:425-432, criterions/OBCCriterion.lua:80-81).

The weights are tests/displaced.py's for `soft`, seed 5, and the table cases are tests/test_gpu_displaced.py's own (computed once per
session): under them the oracle's past flow differs from its future flow by at least 2.75 px on every pixel of the 2 x 128 x 192 case, and
every test asserts >= 1 px on >= 90 % of the pixels before anything else, so a past flow that is really the future flow cannot pass.
Expected values: the CPU oracle (1e-3, the bar of test_gpu_displaced.py), Model.forward's table entry, the entries without the past
flow (bit for bit), the numpy rescale of the network's planes, b2f_flow_warp_past_host (which tests/test_past_flow_cpu.py holds
against the oracle's warp and a numpy restatement) and oracle.warping_unit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, flow_io, ops
from oracle import oracle as O
from tests import displaced as D
from tests import flow_warp_fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_displaced import BAR, SEED, _table_case  # noqa: E402  (the displaced weights, the oracle's and Model.forward's tables)
from tests.test_gpu_float_outputs import _nearest  # noqa: E402  (the index rule of image.scale 'simple' in numpy)
from tests.test_past_flow_cpu import past_field  # noqa: E402

SIZES = [(2, 128, 192), (1, 192, 320)]     # 128 x 192: the level-7 map is 2 x 3
UFS3, UBFS3, OCC3 = (D.table_index(True, 3, w) for w in ("ufs", "ubfs", "occs"))
SOFT, HARD = "random:soft:%d:2.0" % SEED, "random:hard:%d:2.0" % SEED


def _eq(a, b, what):
    """bit-for-bit equality"""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    x, y = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
    if not np.array_equal(x, y):
        d = np.flatnonzero(x != y)
        raise AssertionError("%s: %d bytes differ, first at byte %d" % (what, d.size, d[0]))


def _apart(flow, past, what):
    """>= 1 px between the two flows on >= 90 % of the pixels (x 20: raw network units)"""
    d = np.hypot(*(past.astype(np.float64) - flow.astype(np.float64)).transpose(1, 0, 2, 3)) * 20.0
    share = float((d >= 1.0).mean())
    print("%s: |past - future| >= 1 px on %.1f %% of the pixels, smallest %.2f px" % (what, 100 * share, float(d.min())))
    assert share >= 0.90, (what, share)


@pytest.fixture(scope="module")
def soft():
    """the displaced Soft model of the 2 x 128 x 192 case"""
    exp = _table_case("soft", *SIZES[0])[2]
    _apart(exp[UFS3], exp[UBFS3], "oracle, 2 x 128 x 192")
    m = back2future.Model(SOFT)
    m.set_weights(_table_case("soft", *SIZES[0])[1])
    yield m
    m.close()


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model(HARD)
    yield m
    m.close()


def _clip(seed, T, H0, W0, kind):
    """unit: arbitrary floats in [0, 1); u8: bytes; unit255: the floats k / 255, which cross the link as bytes"""
    r = np.random.default_rng(seed)
    if kind == "unit":
        return r.random((T, 3, H0, W0), dtype=np.float32)
    v = r.integers(0, 256, (T, 3, H0, W0), dtype=np.uint8)
    return v if kind == "u8" else v.astype(np.float32) / np.float32(255)


def _triplets(V):
    return [np.ascontiguousarray(a) for a in (V[:-2], V[1:-1], V[2:])]


def _dev(shape, dtype=torch.float32):
    return torch.full(shape, 7, dtype=dtype, device="cuda")


def _forward(m, d_in, B, H, W, past, unit=False):
    """(flow, occ, est3[, past]) of forward_device as numpy arrays, from buffers filled with sevens"""
    outs = [_dev((B, 2, H, W)) for _ in range(4 if past else 3)]
    torch.cuda.synchronize()
    m.forward_device(d_in.data_ptr(), B, H, W, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), unit_input=unit,
                     d_past_flow=outs[3].data_ptr() if past else None)
    m.synchronize()
    return [o.cpu().numpy() for o in outs]


# ---- 1. the pruned forward pass ----

@pytest.mark.parametrize("B,H,W", SIZES)
def test_forward_device_past_is_the_tables_past_flow(B, H, W):
    x, flat, exp, table = _table_case("soft", B, H, W)
    _apart(exp[UFS3], exp[UBFS3], "oracle, %d x %d x %d" % (B, H, W))
    m = back2future.Model(SOFT)
    try:
        m.set_weights(flat)
        d_in = torch.from_numpy(x).cuda()
        plain = _forward(m, d_in, B, H, W, False)
        flow, occ, est3, past = _forward(m, d_in, B, H, W, True)
        err = float(np.abs(past.astype(np.float64) - exp[UBFS3]).max())
        print("%d x %d x %d: max|past - oracle's skip_ubfs[3]| = %.3g (max|oracle| = %.3g)" % (B, H, W, err, float(np.abs(exp[UBFS3]).max())))
        assert np.isfinite(past).all() and err <= BAR
        _eq(past, table[UBFS3], "past flow vs Model.forward's skip_ubfs[3]")
        for a, b, nm in zip((flow, occ, est3), plain, ("flow", "skip_occs[3]", "est3")):
            _eq(a, b, nm + " with and without the past chain")
        _eq(flow, table[UFS3], "flow vs Model.forward's skip_ufs[3]")
        _eq(occ, table[OCC3], "skip_occs[3] vs Model.forward's")
        # the past flow alone, and a pass without it afterwards
        only = _dev((B, 2, H, W))
        m.forward_device(d_in.data_ptr(), B, H, W, d_past_flow=only.data_ptr())
        m.synchronize()
        _eq(only.cpu().numpy(), past, "the past flow alone")
        for a, b in zip(_forward(m, d_in, B, H, W, False), plain):
            _eq(a, b, "a pass without the past chain after one with it")
    finally:
        m.close()


# ---- 2. sequences, graphs ----

def _sequence(m, frames, T, H, W, past):
    outs = [_dev((T - 2, 2, H, W)) for _ in range(4 if past else 3)]
    torch.cuda.synchronize()
    m.forward_sequence_device(frames.data_ptr(), T, H, W, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                              in_kind=back2future.IN_NORMALIZED, d_past_flow=outs[3].data_ptr() if past else None)
    m.synchronize()
    return outs


def test_sequence_past_equals_the_triplets_and_graphs_stay_apart(soft):
    T, H, W = 5, 128, 192
    f = torch.randn((T, 3, H, W), generator=torch.Generator().manual_seed(11)).cuda()
    x = torch.cat([f[:-2], f[1:-1], f[2:]], dim=1).contiguous()
    tri = _forward(soft, x, T - 2, H, W, True)
    _apart(tri[0], tri[3], "T = 5 sequence")
    seq = [o.cpu().numpy() for o in _sequence(soft, f, T, H, W, True)]
    for a, b, nm in zip(seq, tri, ("flow", "skip_occs[3]", "est3", "past flow")):
        _eq(a, b, "sequence vs overlapping triplets: " + nm)
    plain = [o.cpu().numpy() for o in _sequence(soft, f, T, H, W, False)]
    for a, b in zip(plain, seq):
        _eq(a, b, "sequence with and without the past chain")
    # eager, capture, replay on one set of pointers -- and a call without the past output on the same pointers in between must
    # neither replay the graph with the chain nor leave its own to a call with it
    outs = [_dev((T - 2, 2, H, W)) for _ in range(4)]
    with soft.options(use_graph=1):
        for rnd in range(3):
            for with_past in (False, True):
                for o in outs:
                    o.fill_(7)
                torch.cuda.synchronize()
                soft.forward_sequence_device(f.data_ptr(), T, H, W, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                             in_kind=back2future.IN_NORMALIZED, d_past_flow=outs[3].data_ptr() if with_past else None)
                soft.synchronize()
                what = "round %d, %s the past output" % (rnd, "with" if with_past else "without")
                for a, b in zip(outs[:3], seq):
                    _eq(a.cpu().numpy(), b, what)
                if with_past:
                    _eq(outs[3].cpu().numpy(), seq[3], what + ": past flow")
                else:
                    assert bool((outs[3] == 7).all()), what + ": the past buffer was written"
        # the triplet entry on pointers of its own
        x_outs = [_dev((T - 2, 2, H, W)) for _ in range(4)]
        for rnd in range(3):
            soft.forward_device(x.data_ptr(), T - 2, H, W, *[o.data_ptr() for o in x_outs[:3]], d_past_flow=x_outs[3].data_ptr())
            soft.synchronize()
            for a, b in zip(x_outs, tri):
                _eq(a.cpu().numpy(), b, "triplets, graph round %d" % rnd)


# ---- 3. the computeFlow boundary ----

def _net_past(m, ims):
    """(flow, past flow) of the network at the /64 size on the input the pipeline builds: the raw [0, 1] planes at /64 sizes, else
    ColorNormalize + image.scale (b2f_op_image_scale(normalize = 1), the pipeline's launch_image_scale)"""
    n, _, H0, W0 = ims[0].shape
    fh, fw = H0 - H0 % 64, W0 - W0 % 64
    x = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32) / (np.float32(255) if a.dtype == np.uint8 else 1) for a in ims], axis=1),
                             dtype=np.float32)
    unit = (fh, fw) == (H0, W0)
    if not unit:
        xs = np.empty((n, 9, fh, fw), np.float32)
        for b in range(n):
            _lib.check(_lib.lib().b2f_op_image_scale(m._h, _lib.fptr(x[b]), 9, H0, W0, 1, _lib.fptr(xs[b]), fh, fw))
        x = xs
    res = _forward(m, torch.from_numpy(x).cuda(), n, fh, fw, True, unit=unit)
    return res[0], res[3]


def _rescaled(net, H0, W0):
    """(float)((double)f * sc) with the nearest-index rule of image.scale 'simple' (back2future.lua:78-84); the planes themselves at /64 sizes"""
    fh, fw = net.shape[-2:]
    if (fh, fw) == (H0, W0):
        return net
    out = _nearest(net, H0, W0).astype(np.float64)
    out[:, 0] *= float(W0) / float(fw)
    out[:, 1] *= float(H0) / float(fh)
    return out.astype(np.float32)


@pytest.mark.parametrize("H0,W0", [(128, 192), (136, 200)])
@pytest.mark.parametrize("kind", ["unit", "u8"])
def test_host_and_device_past_entries(soft, H0, W0, kind):
    T = 5
    n = T - 2
    V = _clip(H0 + 1, T, H0, W0, kind)
    ims = _triplets(V)
    what = "%dx%d %s" % (H0, W0, kind)
    f32 = soft.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True)            # flow, fwd, bwd, occ_prob
    net_flow, net_past = _net_past(soft, ims)
    _apart(net_flow, net_past, what + ", network")
    want_past = _rescaled(net_past, H0, W0)
    _eq(_rescaled(net_flow, H0, W0), f32[0], what + ": the rescale rule reproduces the f32 flow")

    def check(res, who):
        flow, past, fwd, bwd, occ = res
        _eq(flow, f32[0], "%s %s: flow" % (what, who))
        _eq(fwd, f32[1], "%s %s: fwd_occ" % (what, who))
        _eq(bwd, f32[2], "%s %s: bwd_occ" % (what, who))
        _eq(occ, f32[3], "%s %s: occ_prob" % (what, who))
        _eq(past, want_past, "%s %s: past flow" % (what, who))

    check(soft.computeFlowBatchPast(*ims, occ_prob=True), "batch")
    check(soft.computeFlowSequencePast(V, occ_prob=True), "sequence")
    with soft.options(host_subbatch_pixels=H0 * W0):                               # one triplet per sub-batch: three of them
        check(soft.computeFlowBatchPast(*ims, occ_prob=True), "batch in three sub-batches")
        check(soft.computeFlowSequencePast(V, occ_prob=True), "sequence in three sub-batches")
    # page-locked buffers, no occ_prob, no masks: DMA in place
    out = tuple(torch.full(s, 7, dtype=torch.float32).pin_memory().numpy() for s in ((n, 2, H0, W0), (n, 2, H0, W0))) + (None, None)
    res = soft.computeFlowSequencePast(V, out=out)
    assert res[0] is out[0] and res[1] is out[1] and res[2] is None and res[3] is None
    _eq(res[0], f32[0], what + " pinned: flow")
    _eq(res[1], want_past, what + " pinned: past flow")
    # the device entries
    d_ims = [torch.from_numpy(a).cuda() for a in ims]
    d_V = torch.from_numpy(np.ascontiguousarray(V)).cuda()
    in_kind = back2future.IN_U8 if kind == "u8" else back2future.IN_UNIT
    for seq in (False, True):
        bufs = [_dev((n, 2, H0, W0)), _dev((n, 2, H0, W0)), _dev((n, 2, H0, W0)), _dev((n, 1, H0, W0), torch.uint8), _dev((n, 1, H0, W0), torch.uint8)]
        torch.cuda.synchronize()
        ptr = [b.data_ptr() for b in bufs]
        if seq:
            soft.computeFlowSequenceDevicePast(d_V.data_ptr(), T, H0, W0, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], in_kind=in_kind)
        else:
            soft.computeFlowDevicePast(*[d.data_ptr() for d in d_ims], n, H0, W0, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], in_kind=in_kind)
        soft.synchronize()
        got = [b.cpu().numpy() for b in bufs]
        check((got[0], got[1], got[3], got[4], got[2]), "device sequence" if seq else "device batch")
    # the f32 entry is what it was
    for a, b in zip(soft.computeFlowBatch(*ims, dtype=np.float32, occ_prob=True), f32):
        _eq(a, b, what + ": the f32 entry after the past calls")


def test_multi_past_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) and a T = 6 sequence on two replicas of one GPU give one context's bits"""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    H0, W0 = 136, 200
    mm = back2future.MultiModel(SOFT, n_gpus=2, devices=[0, 0])
    ref = back2future.Model(SOFT)
    try:
        assert mm.n_gpus == 2
        V = _clip(90, 6, H0, W0, "u8")
        ims = _triplets(V[:5])
        exp = ref.computeFlowBatchPast(*ims, occ_prob=True)
        _eq(exp[1], _rescaled(_net_past(ref, ims)[1], H0, W0), "one context: past flow")
        assert not np.array_equal(exp[0], exp[1])
        for a, b in zip(mm.computeFlowBatchPast(*ims, occ_prob=True), exp):
            _eq(a, b, "batch on two replicas")
        for a, b in zip(mm.computeFlowSequencePast(V, occ_prob=True), ref.computeFlowSequencePast(V, occ_prob=True)):
            _eq(a, b, "sequence on two replicas")
        got = mm.computeFlowSequenceWarp(V, own_past_flow=True, want_past=True)
        want = ref.computeFlowSequenceWarp(V, own_past_flow=True, want_past=True)
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            _eq(a, b, "sequence warp with the own past flow on two replicas")
    finally:
        mm.close()
        ref.close()


# ---- 4. motion compensation with the model's own past flow ----

@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 61), (128, 192)])
def test_device_warp_equals_the_host_entry(soft, H, W, kind):
    """b2f_op_flow_warp_past and b2f_flow_warp_past_device (float in / float out, byte in / byte out) against
    b2f_flow_warp_past_host on the fields of tests/flow_warp_fields.py; the two mixed kernels run in
    test_compute_flow_warp_with_the_own_past_flow, through the pipeline, which alone launches them."""
    flow, ims, prob = F.fields(H, W, kind=kind)
    past = past_field(H, W)
    n = flow.shape[0]
    what = "%dx%d %s" % (H, W, kind)
    for use_prob in (True, False):
        p = prob if use_prob else None
        w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=p, own_past_flow=True, past_flow=past)
        w_got, p_got = ops.flow_warp(flow, *ims, occ_prob=p, own_past_flow=True, past_flow=past, model=soft)
        _eq(w_got, w_want, "%s occ_prob=%d: warped" % (what, use_prob))
        _eq(p_got, p_want, "%s occ_prob=%d: words" % (what, use_prob))
    assert not np.array_equal(p_want, ops.flow_warp(flow, *ims, want_warped=False)[1])
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (flow, past, prob) + tuple(ims)]
    for use_warped, use_photo in ((True, True), (True, False), (False, True)):
        warped = _dev((n, 2, 3, H, W), torch.uint8 if kind == "u8" else torch.float32)
        photo = _dev((n, 14), torch.int64)
        torch.cuda.synchronize()
        soft.flowWarpDevice(d[0].data_ptr(), n, H, W, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                            d_warped=warped.data_ptr() if use_warped else None, d_photo=photo.data_ptr() if use_photo else None,
                            d_occ_prob=d[2].data_ptr(), as_bytes=kind == "u8", own_past_flow=True, d_past_flow=d[1].data_ptr())
        soft.synchronize()
        w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=prob, own_past_flow=True, past_flow=past)
        if use_warped:
            _eq(warped.cpu().numpy(), w_want, what + " device entry: warped")
        if use_photo:
            _eq(photo.cpu().numpy().view(np.uint64), p_want, what + " device entry: words")


@pytest.mark.parametrize("B,H,W", SIZES[:1])
def test_past_planes_are_the_references_warped_img_1(soft, B, H, W):
    """On the normalized frames the network sees, direction 0 is oracle.warping_unit(frame 1, past flow, -20): pwc.lua:425-432 at level 3"""
    x = _table_case("soft", B, H, W)[0]
    flow, occ, est3, past = _forward(soft, torch.from_numpy(x).cuda(), B, H, W, True)
    _apart(flow, past, "GPU, %d x %d x %d" % (B, H, W))
    ims = [np.ascontiguousarray(x[:, 3 * i:3 * i + 3]) for i in range(3)]
    warped = ops.flow_warp(flow, *ims, want_photo=False, own_past_flow=True, past_flow=past, model=soft)[0]
    assert np.isfinite(past).all()
    _eq(warped[:, 0], O.warping_unit(ims[0], past, -20.0), "d = 0 planes vs oracle.warping_unit(frame1, gpu_past_flow, -20)")
    _eq(warped[:, 1], O.warping_unit(ims[2], flow, 20.0), "d = 1 planes vs oracle.warping_unit(frame3, gpu_flow, 20)")
    assert not np.array_equal(warped[:, 0], O.warping_unit(ims[0], flow, -20.0))


@pytest.mark.parametrize("H0,W0,kind", [(128, 192, "unit255"), (136, 200, "u8"), (128, 192, "u8"), (136, 200, "unit")])
def test_compute_flow_warp_with_the_own_past_flow(soft, H0, W0, kind):
    """computeFlow*Warp(own_past_flow=True) is ops.flow_warp of the _past entry's outputs.  unit255 at a /64 size: a sequence's
    frames cross the link as bytes and are sampled as bytes, the warped frames are floats; u8 at 136 x 200: the bytes are unpacked
    for image.scale and sampled as floats, the warped frames are bytes -- with the other two cases all four kernels run."""
    T = 6
    V = _clip(H0 + 3, T, H0, W0, kind)
    ims = _triplets(V)
    what = "%dx%d %s" % (H0, W0, kind)
    flow, past, fo, bo, prob = soft.computeFlowSequencePast(V, occ_prob=True)
    _apart(flow, past, what)
    w_want, p_want = ops.flow_warp(flow, *ims, occ_prob=prob, own_past_flow=True, past_flow=past)
    w_plain, p_plain = soft.computeFlowSequenceWarp(V)
    assert not np.array_equal(p_want[:, 0::2], p_plain[:, 0::2])
    _eq(np.ascontiguousarray(p_want[:, 1::2]), np.ascontiguousarray(p_plain[:, 1::2]), what + ": the future half is the plain entry's")
    w, p = soft.computeFlowSequenceWarp(V, own_past_flow=True)
    _eq(w, w_want, what + " sequence: warped")
    _eq(p, p_want, what + " sequence: words")
    w, p = soft.computeFlowBatchWarp(*ims, own_past_flow=True)
    _eq(w, w_want, what + " batch: warped")
    _eq(p, p_want, what + " batch: words")
    _eq(soft.computeFlowSequenceWarp(V, want_warped=False, own_past_flow=True), p_want, what + " sequence, photo alone")
    with soft.options(host_subbatch_pixels=4 * H0 * W0):     # 4 frames = 2 triplets of a sequence, 4 triplets of a batch
        for pinned in (False, True):
            def buf(shape, dt):
                t = torch.full(shape, 7, dtype=dt)
                return (t.pin_memory() if pinned else t).numpy()
            out = (buf((T - 2, 2, 3, H0, W0), torch.uint8 if kind == "u8" else torch.float32), buf((T - 2, 14), torch.int64).view(np.uint64),
                   buf((T - 2, 2, H0, W0), torch.float32), buf((T - 2, 1, H0, W0), torch.uint8), buf((T - 2, 1, H0, W0), torch.uint8),
                   buf((T - 2, 2, H0, W0), torch.float32), buf((T - 2, 2, H0, W0), torch.float32))
            for call in (lambda: soft.computeFlowSequenceWarp(V, want_flow=True, want_masks=True, want_prob=True, out=out, own_past_flow=True, want_past=True),
                         lambda: soft.computeFlowBatchWarp(*ims, want_flow=True, want_masks=True, want_prob=True, out=out, own_past_flow=True, want_past=True)):
                for a in out:
                    a[...] = 7
                res = call()
                assert len(res) == 7 and all(a is b for a, b in zip(res, out))
                for a, b, nm in zip(res, (w_want, p_want, flow, fo, bo, prob, past), ("warped", "words", "flow", "fwd_occ", "bwd_occ", "occ_prob", "past flow")):
                    _eq(a, b, "%s pinned=%d sub-batched, all outputs: %s" % (what, pinned, nm))
    # the plain warp entry is what it was
    w, p = soft.computeFlowSequenceWarp(V)
    _eq(w, w_plain, what + ": the plain warp entry afterwards")
    _eq(p, p_plain, what + ": the plain warp entry afterwards, words")


# ---- 5. refusals ----

def test_a_hard_model_and_a_stream_are_refused(hard, monkeypatch):
    H0, W0, T = 128, 192, 4
    n = T - 2
    V = _clip(5, T, H0, W0, "unit")
    ims = _triplets(V)
    before = hard.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    d_V = torch.from_numpy(V).cuda()
    d_ims = [torch.from_numpy(a).cuda() for a in ims]
    x = torch.cat(d_ims, dim=1).contiguous()
    bufs = [_dev((n, 2, H0, W0)) for _ in range(3)]
    p = [b.data_ptr() for b in bufs]
    calls = {
        "forward_device": lambda: hard.forward_device(x.data_ptr(), n, H0, W0, p[0], d_past_flow=p[1], unit_input=True),
        "forward_sequence_device": lambda: hard.forward_sequence_device(d_V.data_ptr(), T, H0, W0, p[0], d_past_flow=p[1], in_kind=back2future.IN_UNIT),
        "computeFlowBatchPast": lambda: hard.computeFlowBatchPast(*ims),
        "computeFlowSequencePast": lambda: hard.computeFlowSequencePast(V),
        "computeFlowDevicePast": lambda: hard.computeFlowDevicePast(*[d.data_ptr() for d in d_ims], n, H0, W0, p[0], p[1]),
        "computeFlowSequenceDevicePast": lambda: hard.computeFlowSequenceDevicePast(d_V.data_ptr(), T, H0, W0, p[0], p[1]),
        "computeFlowBatchWarp": lambda: hard.computeFlowBatchWarp(*ims, own_past_flow=True),
        "computeFlowSequenceWarp": lambda: hard.computeFlowSequenceWarp(V, own_past_flow=True, want_past=True),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.B2FError, match="no past-flow decoders"):
            call()
        hard.synchronize()
        assert all(bool((b == 7).all()) for b in bufs), name + ": a refusal wrote an output"
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    mm = back2future.MultiModel(HARD, n_gpus=2, devices=[0, 0])
    try:
        for call in (lambda: mm.computeFlowBatchPast(*ims), lambda: mm.computeFlowSequencePast(V),
                     lambda: mm.computeFlowBatchWarp(*ims, own_past_flow=True), lambda: mm.computeFlowSequenceWarp(V, own_past_flow=True)):
            with pytest.raises(_lib.B2FError, match="no past-flow decoders"):
                call()
    finally:
        mm.close()
    # want_past belongs to the own-past-flow entries
    with pytest.raises(ValueError, match="own_past_flow"):
        hard.computeFlowSequenceWarp(V, want_past=True)
    # a stream's pushes take the f32 and rgb outputs alone: no push carries a past-flow request
    assert not any("past" in name.lower() for name in dir(back2future.FlowStream))
    # the context works afterwards
    for a, b in zip(hard.computeFlowSequence(V, dtype=np.float32, occ_prob=True), before):
        _eq(a, b, "the Hard context after the refusals")


def test_refusals_of_a_soft_context(soft):
    H0, W0 = 128, 192
    V = _clip(6, 3, H0, W0, "unit")
    L = _lib.lib()
    flow = np.zeros((1, 2, H0, W0), np.float32)
    d_past = _dev((1, 2, H0, W0))
    # device memory where host buffers belong, and the reverse
    rc = L.b2f_compute_flow_sequence_past(soft._h, 3, back2future.IN_UNIT, V.ctypes.data, H0, W0, _lib.fptr(flow),
                                          _lib.C.cast(d_past.data_ptr(), _lib.c_float_p), None, None, None)
    assert rc != 0 and "device memory passed to a host-buffer entry point" in L.b2f_last_error().decode()
    d_V, d_flow = torch.from_numpy(V).cuda(), _dev((1, 2, H0, W0))
    with pytest.raises(_lib.B2FError, match="host memory"):
        soft.computeFlowSequenceDevicePast(d_V.data_ptr(), 3, H0, W0, d_flow.data_ptr(), flow.ctypes.data & ~15)
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        soft.computeFlowSequenceDevicePast(d_V.data_ptr(), 3, H0, W0, d_flow.data_ptr(), d_past.data_ptr() + 4)
    x = torch.cat([d_V[:1], d_V[1:2], d_V[2:]], dim=1).contiguous()
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        soft.forward_device(x.data_ptr(), 1, H0, W0, d_flow.data_ptr(), d_past_flow=d_past.data_ptr() + 4, unit_input=True)
    # a context made with b2f_init_ex options: the batch entry runs through the generic executor's table, the sequence entry is refused
    ex = back2future.Model("random:soft", graph="win=5")
    try:
        V4 = _clip(7, 4, 136, 200, "u8")
        ims = _triplets(V4)
        f32 = ex.computeFlowBatch(*ims, dtype=np.float32)
        res = ex.computeFlowBatchPast(*ims)
        _eq(res[0], f32[0], "a generic-graph context: flow")
        assert np.isfinite(res[1]).all() and not np.array_equal(res[0], res[1])
        with pytest.raises(_lib.B2FError, match="shipped graph"):
            ex.computeFlowSequencePast(V4)
    finally:
        ex.close()


# ---- 6. the examples ----

def test_example_flags_on_a_six_frame_clip(tmp_path):
    from PIL import Image
    r = np.random.default_rng(13)
    src, out_seq, out_comp = tmp_path / "frames", tmp_path / "flows", tmp_path / "warped"
    src.mkdir()
    names = ["f%02d" % t for t in range(6)]
    frames = r.integers(0, 256, (6, 128, 192, 3), dtype=np.uint8)
    for nm, f in zip(names, frames):
        Image.fromarray(f).save(str(src / (nm + ".png")))
    V = np.ascontiguousarray(frames.transpose(0, 3, 1, 2))
    m = back2future.Model(SOFT)
    try:
        flow, past, fwd, bwd = m.computeFlowSequencePast(V.astype(np.float32) / np.float32(255))
        warped, photo = m.computeFlowSequenceWarp(V, own_past_flow=True)
        plain = m.computeFlowSequenceWarp(V, want_warped=False)
    finally:
        m.close()
    assert not np.array_equal(photo, plain)
    subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_sequence.py"), str(src), str(out_seq), SOFT, "--past-flow"],
                   check=True, timeout=300, capture_output=True)
    for i, nm in enumerate(names[1:-1]):
        _eq(flow_io.loadFLO(str(out_seq / (nm + "_past.flo"))), past[i], nm + "_past.flo")
        _eq(flow_io.loadFLO(str(out_seq / (nm + ".flo"))), flow[i], nm + ".flo")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "compensate.py"), str(src), str(out_comp), SOFT, "--own-past-flow"],
                       check=True, timeout=300, capture_output=True)
    printed = dict(line.split(" ", 1) for line in p.stdout.decode().splitlines())
    for k, v in back2future.photo_summary(photo).items():
        assert printed[k] == repr(v), (k, printed[k], v)
    for i, nm in enumerate(names[1:-1]):
        for d, tail in enumerate(("_past.png", "_future.png")):
            _eq(np.asarray(Image.open(str(out_comp / (nm + tail))), np.uint8).transpose(2, 0, 1), warped[i, d], nm + tail)
