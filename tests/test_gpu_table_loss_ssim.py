"""GPU: the occlusion-aware SSIM + L1 photometric term (criterions/OSSIML1Criterion.lua; include/b2f.h, B2F_LOSS_SSIM_*) on the device.
b2f_op_table_loss_ssim against the host entry b2f_table_loss_ssim_host (which tests/test_table_loss_ssim_cpu.py holds against a numpy
restatement of the definition): all 32 words of every record equal in the three range modes -- the per-pixel arithmetic is fp64
without contraction, the window has one fixed order, the sums are integers and the range is an integer minimum and maximum, so no
tolerance is involved anywhere -- and words 0 .. 15 are those of b2f_op_table_loss.  Everything above the kernels is defined from
them: Model.forwardLoss(objective="ssim") gives ops.table_loss(objective="ssim") of the table Model.forward returns and of the centre
frame, however the request is cut or sharded where the range does not depend on the cut, and is refused where it would."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops
from tests import table_loss_fields as TL
from tests import table_loss_ssim_fields as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MEAN = np.array([0.485, 0.456, 0.406] * 3, np.float32).reshape(1, 9, 1, 1)
STD = np.array([0.229, 0.224, 0.225] * 3, np.float32).reshape(1, 9, 1, 1)
# The launch caps the grid of one image at 1024 blocks of 256 threads, a thread per group of four pixels of a row: 262144 groups.
# 481 rows of 545 groups (2177 columns, an odd width: scalar loads) are 262145 groups: the first thread alone takes a second one.
WRAP = (481, 2177, 1, 1)
GUARD = 4096


@pytest.fixture(scope="module")
def models():
    m = {False: back2future.Model("random:hard:5:2.0"), True: back2future.Model("random:soft:5:2.0")}
    yield m
    for v in m.values():
        v.close()


def _input(seed, n, H, W):
    r = np.random.default_rng(seed)
    return ((r.random((n, 9, H, W), dtype=np.float32) + (-MEAN)) / STD).astype(np.float32)


def _words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        b, j, k = np.argwhere(got != want)[0]
        raise AssertionError("%s: image %d level %d word %d is %d, expected %d" % (what, b, j, k, got[b, j, k], want[b, j, k]))


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _given(L):
    """a range per level that holds the fields' values without being anyone's own"""
    return np.array([[-3.0 - 0.25 * j, 3.5 + 0.125 * j] for j in range(L)], np.float32)


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L,n", [(1, 1, 1, 2), (1, 5, 1, 2), (5, 1, 1, 2), (2, 3, 1, 2), (3, 3, 1, 2), (4, 4, 1, 2), (5, 7, 1, 2), (37, 53, 1, 2),
                                     (16, 16, 5, 2), (48, 80, 5, 2), WRAP])
def test_op_table_loss_ssim_matches_the_host_entry(models, H, W, L, n, past):
    """Levels of one pixel, one row and one column (the window is all replication), odd sizes (rows and planes start at addresses that
    are no multiple of 16 bytes: scalar loads and scalar heads and tails of the range pass; rows end in a partial group), (16,16,5)
    ends in a 1 x 1 level, (48,80,5) has widths 80 .. 5, and one image with one group more than the capped grid has threads.  The
    tables hold NaN and Inf flows, exact 0 / 0.5 / 1 probabilities and a NaN in the reference image, which its neighbours' windows see."""
    table, ref = TL.tables(H, W, L, past, n=n)
    if n > 1:
        for t in table:     # the second image on another range: the batch's range is not each image's own
            t[1] *= np.float32(0.5)
    modes = [("batch", "batch"), ("image", "image"), ("given", _given(L))] if (H, W, L, n) != WRAP else [("image", "image")]
    for name, rng in modes:
        want = ops.table_loss(table, ref, objective="ssim", ssim_range=rng)
        got = ops.table_loss(table, ref, model=models[past], objective="ssim", ssim_range=rng)
        assert got.shape == (n, L, 32)
        _words(got, want, "%dx%d L=%d %s" % (H, W, L, name))
    _words(got[:, :, :16].copy(), ops.table_loss(table, ref, model=models[past]), "%dx%d L=%d words 0 .. 15" % (H, W, L))
    assert not got[:, :, 26:].any()
    if (H, W, L, n) != WRAP:
        half = ops.table_loss(table, ref, flow_scale=10.0, model=models[past], objective="ssim", ssim_range="batch")
        _words(half, ops.table_loss(table, ref, flow_scale=10.0, objective="ssim", ssim_range="batch"), "%dx%d L=%d flow_scale=10" % (H, W, L))


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_device_entry_on_a_side_stream_right_behind_the_uploads(models, past):
    H, W, L, n = 48, 80, 3, 2
    table, ref = TL.tables(H, W, L, past, n=n, seed=3)
    m = models[past]
    stream = torch.cuda.Stream()
    loss = torch.full((n, L, 32), 7, dtype=torch.int64, device="cuda")
    pinned = [torch.from_numpy(t).pin_memory() for t in table + [ref]]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dev = [t.to("cuda", non_blocking=True) for t in pinned]
        for rng in ("batch", "image", _given(L)):
            m.tableLossDevice([d.data_ptr() for d in dev[:-1]], n, H, W, dev[-1].data_ptr(), loss.data_ptr(), stream=stream.cuda_stream, objective="ssim",
                              ssim_range=rng)
            stream.synchronize()
            _words(loss.cpu().numpy().view(np.uint64), ops.table_loss(table, ref, objective="ssim", ssim_range=rng), "device entry")
    loss.fill_(7)
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() for d in dev[:-1]]
    with pytest.raises(_lib.B2FError, match="b2f_table_loss_ssim_device: device buffers must be 16-byte aligned"):
        m.tableLossDevice([ptrs[0] + 4] + ptrs[1:], n, H, W, dev[-1].data_ptr(), loss.data_ptr(), objective="ssim")
    with pytest.raises(_lib.B2FError, match="host memory"):
        m.tableLossDevice(ptrs, n, H, W, ref.ctypes.data & ~15, loss.data_ptr(), objective="ssim")
    with pytest.raises(_lib.B2FError, match="n_outs"):
        m.tableLossDevice(ptrs[:7], n, H, W, dev[-1].data_ptr(), loss.data_ptr(), objective="ssim")
    cptrs = (C.c_void_p * len(ptrs))(*[C.c_void_p(p) for p in ptrs])
    entry = _lib.lib().b2f_table_loss_ssim_device
    assert entry(m._h, cptrs, len(ptrs), n, H, W, C.c_void_p(dev[-1].data_ptr()), 20.0, C.c_void_p(loss.data_ptr()), None, 3, None) != 0
    assert "range_mode" in _lib.lib().b2f_last_error().decode()
    assert entry(m._h, cptrs, len(ptrs), n, H, W, C.c_void_p(dev[-1].data_ptr()), 20.0, C.c_void_p(loss.data_ptr()), None, SS.GIVEN, None) != 0
    assert "ranges" in _lib.lib().b2f_last_error().decode()
    torch.cuda.synchronize()
    assert (loss.cpu().numpy() == 7).all()        # a refused call writes nothing


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_forward_loss_ssim_is_the_table_loss_ssim_of_forward(models, past):
    """128 x 192, n = 3: the records of the table that never left the GPU are those of the downloaded one; want_table returns
    Model.forward's bits; three sub-batches of one triplet give the same words and the same table with the image's own and with a given
    range; the batch's range is served whole and refused when cut, with nothing written."""
    m = models[past]
    x = _input(43 + past, 3, 128, 192)
    table = m.forward(x)
    given = _given(5)
    want = {"image": ops.table_loss(table, x[:, 3:6], objective="ssim", ssim_range="image"),
            "batch": ops.table_loss(table, x[:, 3:6], objective="ssim", ssim_range="batch"),
            "given": ops.table_loss(table, x[:, 3:6], objective="ssim", ssim_range=given)}
    assert want["image"].shape == (3, 5, 32)
    assert want["image"][:, :, SS.SSIM:SS.SSIM + 4].all() and not want["image"][:, :, SS.SSIM_NONFINITE:SS.SSIM_NONFINITE + 2].any()
    assert not np.array_equal(want["image"], want["batch"])
    rng = {"image": "image", "batch": "batch", "given": given}
    for k in ("image", "batch", "given"):
        _words(m.forwardLoss(x, objective="ssim", ssim_range=rng[k]), want[k], "forwardLoss " + k)
    rec, tab = m.forwardLoss(x, want_table=True, objective="ssim", ssim_range="image")
    _words(rec, want["image"], "forwardLoss with the table")
    assert len(tab) == len(table) == (25 if past else 20)
    for i, (a, b) in enumerate(zip(tab, table)):
        _eq(a, b, "table tensor %d" % i)
    with m.options(host_subbatch_pixels=128 * 192):
        for k in ("image", "given"):
            _words(m.forwardLoss(x, objective="ssim", ssim_range=rng[k]), want[k], "three sub-batches " + k)
        rec, tab = m.forwardLoss(x, want_table=True, objective="ssim", ssim_range="image")
        _words(rec, want["image"], "three sub-batches with the table")
        for i, (a, b) in enumerate(zip(tab, table)):
            _eq(a, b, "three sub-batches: table tensor %d" % i)
        # the batch's range on a request that would be cut: refused, the message names the other two modes, nothing written
        out = np.full((3, 5, 32), 7, np.uint64)
        rc = _lib.lib().b2f_forward_loss_ssim(m._h, _lib.fptr(x), 3, 128, 192, 20.0, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), None, 0, SS.BATCH, None)
        msg = _lib.lib().b2f_last_error().decode()
        assert rc != 0 and "b2f_forward_loss_ssim: B2F_SSIM_RANGE_BATCH" in msg and "B2F_SSIM_RANGE_IMAGE" in msg and "B2F_SSIM_RANGE_GIVEN" in msg
        assert (out == 7).all()
        loss = torch.full((3, 5, 32), 7, dtype=torch.int64, device="cuda")
        dx = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        with pytest.raises(_lib.B2FError, match="b2f_forward_loss_ssim_device: B2F_SSIM_RANGE_BATCH"):
            m.forwardLossDevice(dx.data_ptr(), 3, 128, 192, loss.data_ptr(), objective="ssim", ssim_range="batch")
        torch.cuda.synchronize()
        assert (loss.cpu().numpy() == 7).all()
    # the device entry on a side stream, behind the upload
    stream = torch.cuda.Stream()
    loss = torch.full((3, 5, 32), 7, dtype=torch.int64, device="cuda")
    px = torch.from_numpy(x).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dx = px.to("cuda", non_blocking=True)
        m.forwardLossDevice(dx.data_ptr(), 3, 128, 192, loss.data_ptr(), stream=stream.cuda_stream, objective="ssim", ssim_range="batch")
    stream.synchronize()
    _words(loss.cpu().numpy().view(np.uint64), want["batch"], "forwardLossDevice")
    with pytest.raises(_lib.B2FError, match="b2f_forward_loss_ssim_device: in_kind must be B2F_IN_NORMALIZED"):
        _lib.check(_lib.lib().b2f_forward_loss_ssim_device(m._h, dx.data_ptr(), back2future.IN_UNIT, 3, 128, 192, 20.0, loss.data_ptr(), None, SS.IMAGE, None))
    with pytest.raises(ValueError):
        m.forwardLoss(x, objective="ssim", ssim_range="clip")
    with pytest.raises(ValueError):
        m.forwardLoss(x, objective="ssim", ssim_range=np.zeros((4, 2), np.float32))


def test_the_default_and_finetune_calls_are_unchanged_by_the_ssim_stage():
    """A context that has run the SSIM stage returns for the default and the "finetune" calls the 16- and 24-word records of a
    context that never did, bit for bit."""
    x = _input(47, 2, 64, 128)
    fresh = back2future.Model("random:soft:5:2.0")
    try:
        base16, base24 = fresh.forwardLoss(x), fresh.forwardLoss(x, objective="finetune")
    finally:
        fresh.close()
    m = back2future.Model("random:soft:5:2.0")
    try:
        rec = m.forwardLoss(x, objective="ssim", ssim_range="image")
        got16, got24 = m.forwardLoss(x), m.forwardLoss(x, objective="finetune")
    finally:
        m.close()
    assert base16.shape == (2, 5, 16) and base24.shape == (2, 5, 24) and rec.shape == (2, 5, 32)
    _words(got16, base16, "default call behind the ssim stage")
    _words(got24, base24, "finetune call behind the ssim stage")
    _words(rec[:, :, :16].copy(), base16, "words 0 .. 15 of the ssim records")


def test_multi_forward_loss_ssim_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) on two replicas of one GPU give one context's words; the batch's range is refused."""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        x = _input(23, 3, 64, 128)
        want = ref.forwardLoss(x, objective="ssim", ssim_range="image")
        assert want.shape == (3, 5, 32) and want[:, :, SS.SSIM].all()
        _words(mm.forwardLoss(x, objective="ssim"), want, "two replicas")
        given = _given(5)
        _words(mm.forwardLoss(x, objective="ssim", ssim_range=given), ref.forwardLoss(x, objective="ssim", ssim_range=given), "two replicas, given range")
        _words(mm.forwardLoss(x), want[:, :, :16].copy(), "two replicas, default arguments")
        with pytest.raises(ValueError):
            mm.forwardLoss(x, objective="ssim", ssim_range="batch")
        out = np.full((3, 5, 32), 7, np.uint64)
        rc = _lib.lib().b2f_multi_forward_loss_ssim(mm._h, _lib.fptr(x), 3, 64, 128, 20.0, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), SS.BATCH, None)
        msg = _lib.lib().b2f_last_error().decode()
        assert rc != 0 and "B2F_SSIM_RANGE_IMAGE" in msg and "B2F_SSIM_RANGE_GIVEN" in msg and (out == 7).all()
    finally:
        mm.close()
        ref.close()


def test_a_context_made_with_options_and_a_two_frame_one():
    """win=5,levels=4,skip=2: a table of two levels from the generic executor; two_frame is refused with nothing written."""
    m = back2future.Model("random:soft:3:2.0", graph="win=5,levels=4,skip=2")
    try:
        x = _input(33, 2, 32, 48)
        table = m.forward(x)
        assert len(table) == 10
        want = ops.table_loss(table, x[:, 3:6], objective="ssim", ssim_range="image")
        assert want.shape == (2, 2, 32)
        _words(m.forwardLoss(x, objective="ssim", ssim_range="image"), want, "win=5,levels=4,skip=2")
        _words(ops.table_loss(table, x[:, 3:6], model=m, objective="ssim", ssim_range="image"), want, "op on the generic table")
    finally:
        m.close()
    m = back2future.Model("random:hard:3:2.0", graph="two_frame=1")
    try:
        x = _input(34, 1, 64, 64)
        with pytest.raises(_lib.B2FError, match="b2f_forward_loss_ssim: a two_frame model"):
            m.forwardLoss(x, objective="ssim", ssim_range="image")
        loss = torch.full((1, 7, 32), 7, dtype=torch.int64, device="cuda")
        dx = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        with pytest.raises(_lib.B2FError, match="b2f_forward_loss_ssim_device: a two_frame model"):
            m.forwardLossDevice(dx.data_ptr(), 1, 64, 64, loss.data_ptr(), objective="ssim", ssim_range="image")
        torch.cuda.synchronize()
        assert (loss.cpu().numpy() == 7).all()
    finally:
        m.close()


def test_the_op_entry_and_forward_loss_under_guards():
    """arena_guard = 4096 floats and arena_fill = 1: the op entry's staging buffers and the forward's arena are guarded and start as a
    NaN pattern; the words are those of a plain context and b2f_arena_check finds every guard word in place."""
    g = back2future.Model("random:soft:5:2.0")
    p = back2future.Model("random:soft:5:2.0")
    try:
        g.set_option("arena_guard", GUARD)
        g.set_option("arena_fill", 1)
        table, ref = TL.tables(37, 53, 1, True)
        for rng in ("batch", "image"):
            _words(ops.table_loss(table, ref, model=g, objective="ssim", ssim_range=rng), ops.table_loss(table, ref, objective="ssim", ssim_range=rng),
                   "guarded op entry " + rng)
            assert g.arena_check() == 0
        x = _input(49, 2, 64, 128)
        want = p.forwardLoss(x, objective="ssim", ssim_range="image")
        _words(g.forwardLoss(x, objective="ssim", ssim_range="image"), want, "guarded forwardLoss")
        assert g.arena_check() == 0
    finally:
        g.close()
        p.close()


def test_validate_example_prints_the_ssim_criterion(tmp_path):
    """examples/validate.py --pme-criterion OSSIML1 on four 70 x 130 PNGs (cropped to 64 x 128): value for value loss_summary of
    Model.forwardLoss(objective="ssim", ssim_range="image") with that criterion."""
    from PIL import Image
    r = np.random.default_rng(15)
    names = ["f%02d" % t for t in range(4)]
    frames = r.integers(0, 256, (4, 70, 130, 3), dtype=np.uint8)
    for nm, f in zip(names, frames):
        Image.fromarray(f).save(str(tmp_path / (nm + ".png")))
    script = os.path.join(ROOT, "examples", "validate.py")
    norm = [back2future.normalize(np.ascontiguousarray(f[:64, :128].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)) for f in frames]
    x = np.stack([np.concatenate(norm[i:i + 3], axis=0) for i in range(2)])
    m = back2future.Model("random:soft:5:2.0")
    try:
        rec = m.forwardLoss(x, objective="ssim", ssim_range="image")
    finally:
        m.close()
    p = subprocess.run([sys.executable, script, str(tmp_path), "random:soft:5:2.0", "--pme-criterion", "OSSIML1"], check=True, timeout=300,
                       capture_output=True)
    printed = dict(line.split(" ", 1) for line in p.stdout.decode().splitlines())
    s = back2future.loss_summary(rec, pme_criterion="OSSIML1")
    assert printed == {"f01": repr(float(s["loss"][0])), "f02": repr(float(s["loss"][1])), "mean": repr(s["mean"]), "nonfinite": "0"}
    assert s["loss"][0] != back2future.loss_summary(rec)["loss"][0] and s["loss"][0] != back2future.loss_summary(rec, pme_criterion="OSSIM")["loss"][0]
    bad = subprocess.run([sys.executable, script, str(tmp_path), "random:soft:5:2.0", "--pme-criterion", "SSIM"], capture_output=True, timeout=300)
    assert bad.returncode != 0 and b"--pme-criterion" in bad.stderr
