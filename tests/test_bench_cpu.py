"""CPU: bench.py --dump-outputs -- arrays under the budget are written whole; above it every array keeps all triplets and
channels at one fixed, seeded set of pixels, the same for every array and every run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import bench  # noqa: E402


def _outs(B, H, W):
    g = torch.Generator().manual_seed(0)
    return {"flow": torch.rand(B, 2, H, W, generator=g), "occ": torch.rand(B, 2, H, W, generator=g), "est3": torch.rand(B, 3, H, W, generator=g)}


def test_dump_small_outputs_whole(tmp_path):
    outs = _outs(2, 16, 24)
    bench.dump_outputs(torch, outs, 16, 24, str(tmp_path))
    for n, t in outs.items():
        a = np.load(str(tmp_path / (n + ".npy")))
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, t.numpy())


def test_dump_large_outputs_as_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 7 * 4 * 50)      # room for 50 of the 16 x 24 pixels of 2 triplets x 7 channels
    outs = _outs(2, 16, 24)
    for d in ("a", "b"):
        bench.dump_outputs(torch, outs, 16, 24, str(tmp_path / d))
    total = sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) - 128 for n in outs)   # less the .npy headers
    assert total <= bench.DUMP_BYTES
    pix = None
    for n, t in outs.items():
        a = np.load(str(tmp_path / "a" / (n + ".npy")))
        np.testing.assert_array_equal(a, np.load(str(tmp_path / "b" / (n + ".npy"))))
        assert a.shape == (2, t.shape[1], 50) and a.dtype == np.float32
        flat = t.reshape(2, t.shape[1], -1).numpy()
        # the sampled pixels are the same positions in every array: recover them from the first one
        where = [int(np.flatnonzero((flat[0, 0] == v))[0]) for v in a[0, 0]]
        if pix is None:
            pix = where
            assert pix == sorted(set(pix))
        np.testing.assert_array_equal(a, flat[:, :, pix])
