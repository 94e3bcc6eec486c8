"""GPU: the step from one work item to the next inside a persistent block of the F(6x6) kernel (csrc/b2f_wino6.hip).

A block decodes its next item (n-block, image, tile row and column) with reciprocal multiplications set by the launcher, and the output
stage of an item leaves the accumulators ready for the next one: zero, and in wave 1 the bias of the NEXT item's n-block.  The shapes
below make one block walk through every kind of step -- another n-block (bias and weight offset move), another image, another tile row
and column with ragged right and bottom edges, the last item of a block (no successor) -- in both block forms (64 and 32 outputs).
Every output has a bias of its own, so a bias taken from the wrong n-block shows."""
import numpy as np
import pytest

from back2future_amd import back2future, ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hard():
    m = back2future.Model("random:hard:5:2.0")
    yield m
    m.close()


# ci, co, images, h, w, persistent blocks
SHAPES = [
    (32, 160, 3, 25, 97, (1, 2, 7)),     # 3 x 3 items per image, ragged both ways; two 64-output blocks (one launch) + the 32-output block
    (64, 32, 3, 13, 50, (1, 3)),         # the 32-output form alone, 2 x 2 items per image with one row and two columns in the ragged ones
    (200, 128, 2, 12, 48, (1, 2, 3, 4)), # one item per image and n-block: every step changes the image (2 blocks) or both (3); 4 blocks: no item has a successor
]


@pytest.mark.parametrize("ci,co,n,h,w,blocks", SHAPES)
def test_wino6_item_steps(hard, ci, co, n, h, w, blocks):
    r = np.random.default_rng(ci * 7 + co)
    x = r.standard_normal((n, ci, h, w), dtype=np.float32)
    wt = (r.standard_normal((co, ci, 3, 3), dtype=np.float32) / np.sqrt(9 * ci)).astype(np.float32)
    b = r.permutation(np.linspace(-2.0, 2.0, co)).astype(np.float32)        # a distinct bias per output
    assert len(set(b.tolist())) == co
    exp = O.conv3x3(x, wt, b, 1, True)
    with hard.options(wino6=0):
        other = ops.conv3x3(hard, x, wt, b, 1, True)
    with hard.options(wino6=1, wino6_min_pixels=0):
        full = ops.conv3x3(hard, x, wt, b, 1, True)                         # the default grid: one block per item up to the CU count
        got = {}
        for k in blocks:
            with hard.options(wino4_persistent=k):                          # values > 1: exactly that many persistent blocks; 1: the default grid
                got[k] = ops.conv3x3(hard, x, wt, b, 1, True)
    assert not np.array_equal(full, other)                                  # the F(6x6) kernel really ran
    # the bars of test_conv3x3_wino6
    np.testing.assert_allclose(full, exp, rtol=1e-4, atol=1.5e-4)
    assert np.abs(full - exp).mean() < 5e-6
    for k in blocks:
        np.testing.assert_allclose(got[k], exp, rtol=1e-4, atol=1.5e-4)
        assert np.array_equal(got[k], full), "persistent blocks = %d" % k
