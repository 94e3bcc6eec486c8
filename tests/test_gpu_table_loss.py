"""GPU: the unsupervised validation loss of test.lua:266-297 on the device.  b2f_op_table_loss against the host entry
b2f_table_loss_host (which tests/test_table_loss_cpu.py holds against a numpy restatement of the definition): all 16 words of every
record equal -- the per-pixel arithmetic is fp64 without contraction and the sums are integers, so no tolerance is involved anywhere.
Everything above the kernel is defined from it: Model.forwardLoss gives ops.table_loss of the table Model.forward returns and of the
centre frame, however the request is cut or sharded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from back2future_amd import _lib, back2future, ops, weights as W
from tests import table_loss_fields as TL
from tests import trained_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MEAN = np.array([0.485, 0.456, 0.406] * 3, np.float32).reshape(1, 9, 1, 1)
STD = np.array([0.229, 0.224, 0.225] * 3, np.float32).reshape(1, 9, 1, 1)


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


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("H,W,L,n", [(1, 1, 1, 2), (2, 3, 1, 2), (37, 53, 1, 2), (16, 16, 5, 2), (48, 80, 5, 2), (64, 64, 5, 2), (1024, 1920, 5, 1)])
def test_op_table_loss_matches_the_host_entry(models, H, W, L, n, past):
    """Odd sizes: rows and planes start at addresses that are no multiple of 16 bytes (scalar loads) and rows end in a partial group;
    (16,16,5) ends in a 1 x 1 level, (48,80,5) has widths 80 .. 5; one 1024 x 1920 image has more groups than the capped grid has
    threads (the loop wraps).  The tables hold whole-pixel and zero flows, targets off every side and exactly on the border, NaN and
    Inf, exact 0 / 0.5 / 1 probabilities, flat runs, ramps, hard edges and a NaN in the reference image."""
    table, ref = TL.tables(H, W, L, past, n=n)
    want = ops.table_loss(table, ref)
    got = ops.table_loss(table, ref, model=models[past])
    _words(got, want, "%dx%d L=%d" % (H, W, L))
    assert (got[:, :, TL.PIXELS] == [(H >> j) * (W >> j) for j in range(L)]).all()
    half = ops.table_loss(table, ref, flow_scale=10.0, model=models[past])
    _words(half, ops.table_loss(table, ref, flow_scale=10.0), "%dx%d L=%d flow_scale=10" % (H, W, L))


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_device_entry_on_a_side_stream_right_behind_the_uploads(models, past):
    H, W, L, n = 48, 80, 3, 2
    table, ref = TL.tables(H, W, L, past, n=n, seed=3)
    m = models[past]
    stream = torch.cuda.Stream()
    loss = torch.full((n, L, 16), 7, dtype=torch.int64, device="cuda")
    pinned = [torch.from_numpy(t).pin_memory() for t in table + [ref]]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dev = [t.to("cuda", non_blocking=True) for t in pinned]
        m.tableLossDevice([d.data_ptr() for d in dev[:-1]], n, H, W, dev[-1].data_ptr(), loss.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _words(loss.cpu().numpy().view(np.uint64), ops.table_loss(table, ref), "device entry")
    with pytest.raises(_lib.B2FError, match="16-byte aligned"):
        m.tableLossDevice([dev[0].data_ptr() + 4] + [d.data_ptr() for d in dev[1:-1]], n, H, W, dev[-1].data_ptr(), loss.data_ptr())
    with pytest.raises(_lib.B2FError, match="host memory"):
        m.tableLossDevice([d.data_ptr() for d in dev[:-1]], n, H, W, ref.ctypes.data & ~15, loss.data_ptr())
    with pytest.raises(_lib.B2FError, match="n_outs"):
        m.tableLossDevice([d.data_ptr() for d in dev[:7]], n, H, W, dev[-1].data_ptr(), loss.data_ptr())


@pytest.mark.parametrize("past", [False, True], ids=["hard", "soft"])
def test_forward_loss_is_the_table_loss_of_forward(models, past):
    """64 x 64, n = 3: the records of the table that never left the GPU are those of the downloaded one; want_table returns
    Model.forward's bits; three sub-batches of one triplet give the same words and the same table."""
    m = models[past]
    x = _input(11 + past, 3, 64, 64)
    table = m.forward(x)
    want = ops.table_loss(table, x[:, 3:6])
    assert want.shape == (3, 5, 16)
    _words(m.forwardLoss(x), want, "forwardLoss")
    _words(ops.table_loss(table, x[:, 3:6], model=m), want, "op on forward's table")
    rec, tab = m.forwardLoss(x, want_table=True)
    _words(rec, want, "forwardLoss with the table")
    assert len(tab) == len(table) == (25 if past else 20)
    for i, (a, b) in enumerate(zip(tab, table)):
        _eq(a, b, "table tensor %d" % i)
    with m.options(host_subbatch_pixels=64 * 64):
        _words(m.forwardLoss(x), want, "three sub-batches")
        rec, tab = m.forwardLoss(x, want_table=True)
        _words(rec, want, "three sub-batches with the table")
        for i, (a, b) in enumerate(zip(tab, table)):
            _eq(a, b, "three sub-batches: table tensor %d" % i)
    _words(m.forwardLoss(x, flow_scale=5.0), ops.table_loss(table, x[:, 3:6], flow_scale=5.0), "flow_scale = 5")
    # the device entry on a side stream, behind the upload
    stream = torch.cuda.Stream()
    loss = torch.full((3, 5, 16), 7, dtype=torch.int64, device="cuda")
    px = torch.from_numpy(x).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dx = px.to("cuda", non_blocking=True)
        m.forwardLossDevice(dx.data_ptr(), 3, 64, 64, loss.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _words(loss.cpu().numpy().view(np.uint64), want, "forwardLossDevice")
    with pytest.raises(_lib.B2FError, match="B2F_IN_NORMALIZED"):
        _lib.check(_lib.lib().b2f_forward_loss_device(m._h, dx.data_ptr(), back2future.IN_UNIT, 3, 64, 64, 20.0, loss.data_ptr(), None))
    with pytest.raises(_lib.B2FError, match="multiples of 64"):
        m.forwardLoss(_input(1, 1, 32, 64))


def test_forward_loss_with_weights_like_trained_ones(capsys):
    """128 x 192, n = 2, a Soft model whose flows span many pixels (tests/trained_like.py); prints the summary kept in
    profiles/r12_table_loss.json."""
    x = _input(1, 2, 128, 192)
    params = trained_like.calibrate(W.random_init(7, True, 1.0), x, True)
    m = back2future.Model("random:soft:1:1.0")
    try:
        m.set_weights(params)
        table = m.forward(x)
        want = ops.table_loss(table, x[:, 3:6])
        _words(m.forwardLoss(x), want, "trained-like forwardLoss")
    finally:
        m.close()
    assert want[:, :, TL.OUTSIDE:TL.OUTSIDE + 2].sum() > 0, "no flow of the trained-like model leaves the image"
    s = back2future.loss_summary(want)
    doc = {"shape": [2, 128, 192], "model": "random:soft:1:1.0 calibrated (tests/trained_like.py)", "like": "test", "size_average": False,
           "records": want.tolist(), "summary": {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()},
           "summary_size_average": {k: (v.tolist() if isinstance(v, np.ndarray) else v)
                                    for k, v in back2future.loss_summary(want, size_average=True).items()}}
    with capsys.disabled():
        print("\nr12_table_loss " + json.dumps(doc))
    assert np.isfinite(s["loss"]).all() and s["mean"] > 0


def test_multi_forward_loss_two_replicas_on_one_gpu(monkeypatch):
    """n = 3 triplets (shards 2 + 1) on two replicas of one GPU give one context's words."""
    monkeypatch.setenv("B2F_MULTI_TRANSPORT", "peer")
    monkeypatch.setenv("B2F_MULTI_ALLOW_DUPLICATE", "1")
    mm = back2future.MultiModel("random:soft:5:2.0", n_gpus=2, devices=[0, 0])
    ref = back2future.Model("random:soft:5:2.0")
    try:
        assert mm.n_gpus == 2
        x = _input(21, 3, 64, 128)
        _words(mm.forwardLoss(x), ref.forwardLoss(x), "two replicas")
    finally:
        mm.close()
        ref.close()


def test_a_context_made_with_options_gives_the_host_entrys_words():
    """win=5,levels=4,skip=2: a table of two levels from the generic executor; two_frame is refused with a message."""
    m = back2future.Model("random:soft:3:2.0", graph="win=5,levels=4,skip=2")
    try:
        x = _input(31, 2, 32, 48)
        table = m.forward(x)
        assert len(table) == 10
        want = ops.table_loss(table, x[:, 3:6])
        assert want.shape == (2, 2, 16)
        _words(m.forwardLoss(x), want, "win=5,levels=4,skip=2")
        _words(ops.table_loss(table, x[:, 3:6], model=m), want, "op on the generic table")
    finally:
        m.close()
    m = back2future.Model("random:hard:3:2.0", graph="two_frame=1")
    try:
        with pytest.raises(_lib.B2FError, match="two_frame"):
            m.forwardLoss(_input(32, 1, 64, 64))
    finally:
        m.close()


def test_validate_example_prints_the_loss_per_centre_frame(tmp_path):
    """examples/validate.py on four 70 x 130 PNGs (cropped to 64 x 128): one line per centre frame, the mean and the non-finite count,
    value for value loss_summary of Model.forwardLoss on the cropped, normalized triplets."""
    from PIL import Image
    r = np.random.default_rng(14)
    names = ["f%02d" % t for t in range(4)]
    frames = r.integers(0, 256, (4, 70, 130, 3), dtype=np.uint8)
    for nm, f in zip(names, frames):
        Image.fromarray(f).save(str(tmp_path / (nm + ".png")))
    script = os.path.join(ROOT, "examples", "validate.py")
    norm = [back2future.normalize(np.ascontiguousarray(f[:64, :128].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)) for f in frames]
    x = np.stack([np.concatenate(norm[i:i + 3], axis=0) for i in range(2)])
    m = back2future.Model("random:soft:5:2.0")
    try:
        rec = m.forwardLoss(x)
    finally:
        m.close()
    for extra, kw in (([], {}), (["--like", "train", "--size-average"], {"like": "train", "size_average": True})):
        p = subprocess.run([sys.executable, script, str(tmp_path), "random:soft:5:2.0"] + extra, check=True, timeout=300, capture_output=True)
        printed = dict(line.split(" ", 1) for line in p.stdout.decode().splitlines())
        s = back2future.loss_summary(rec, **kw)
        assert printed == {"f01": repr(float(s["loss"][0])), "f02": repr(float(s["loss"][1])), "mean": repr(s["mean"]), "nonfinite": "0"}
