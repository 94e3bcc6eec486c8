"""GPU: the workspace as the test -- guard bands around every buffer of the arena, and a recognisable NaN in every byte that a kernel
has no business touching (options arena_guard / arena_fill, b2f_arena_check; DESIGN.md section 5, "Guards").

The contract: a kernel may read outside its tensors only if the value cannot reach a result, and may write nowhere outside them.  Every
case here runs one context with arena_guard = 4096 floats and arena_fill = 1 (arena and stream block start as 0x7fc0a5a5, a quiet NaN)
against a second context with both at 0, on the same weights and inputs.  The outputs must be bit-identical -- a NaN that reaches
arithmetic does not stay hidden: a select discards it, a multiplication by zero does not -- and b2f_arena_check must find every guard
word as it was written, after every call.

What the guard width can and cannot see: 4096 floats is a condition, not a measurement.  It is more than the longest contiguous piece a
kernel here stores in one go (an F(6x6) item row: 48 pixels x 8 floats = 384; a record row piece: 128) and more than a whole level-3 row
of these sizes (80 pixels x 8 floats), so an overrun by such a piece or row lands in a guard.  An overrun longer than the guard, or a stray
access with a stride that steps over it, reaches the next buffer and may go unseen; so does a stray write of the very bits the guard
holds, and a stray read whose value a select throws away (which the contract allows).

Covered here: the shipped graph's plans -- the full table (with b2f_forward's output tensors as guarded buffers), the pruned pass eager,
captured and replayed, sequences, streams, a warm context.  The generic executor of the other option sets (graph_run, its own layout of
the arena with a guard behind every buffer, named by role and level) is held to the same contract in tests/test_gpu_graph_guards.py.

The op-level entries (b2f_op_*) carry the same guards on every device buffer, always on: the shapes of test_gpu_parity.py,
test_gpu_in_place.py and test_gpu_cv_float64.py are that coverage.  The self-test at the end shows both detectors firing on one word
overwritten from the host."""
import functools

import numpy as np
import pytest

from back2future_amd import _lib, back2future

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_displaced import KERNEL_SETTINGS, SEED, _table_case  # noqa: E402
from tests.test_gpu_sequence import _outs  # noqa: E402

GUARD = 4096
KINDS = ["hard", "soft"]
SIZES = [(1, 64, 64), (2, 128, 192), (1, 192, 320)]     # level 7: 1 x 1, 2 x 3 and 3 x 5 maps; 192 x 320: odd sizes at every coarse level
SETTINGS = ["default"] + list(KERNEL_SETTINGS)


@functools.lru_cache(maxsize=None)
def _case(which, B, H, Wd):
    """(x, weights): the table case of tests/test_gpu_displaced.py where it has the size.  1 x 64 x 64: input drawn the same way, on the
    weights of the 2 x 128 x 192 case -- displaced.py calibrates each occlusion head on the inter-quartile range of its logits, which a
    level-7 map of one pixel does not have; the flow biases, which move the warps through the clamp, do not depend on the input."""
    past = which == "soft"
    if (B, H, Wd) != (1, 64, 64):
        return _table_case(which, B, H, Wd)[:2]
    x = np.random.default_rng(H + Wd + past).standard_normal((B, 9, H, Wd)).astype(np.float32)
    return x, _table_case(which, 2, 128, 192)[1]


def _guarded(name):
    m = back2future.Model(name)
    m.set_option("arena_guard", GUARD)
    m.set_option("arena_fill", 1)
    return m


_pairs = {}


def _pair(which, flat=None, key=None):
    """(guarded context, plain context) of a model kind, both on weights `flat` (reloaded when `key` changes)"""
    g, p, k = _pairs.get(which, (None, None, None))
    if g is None:
        g, p = _guarded("random:%s:%d:2.0" % (which, SEED)), back2future.Model("random:%s:%d:2.0" % (which, SEED))
    if flat is not None and k != key:
        g.set_weights(flat)
        p.set_weights(flat)
        k = key
    _pairs[which] = (g, p, k)
    assert g.get_option("arena_guard") == GUARD and g.get_option("arena_fill") == 1
    assert p.get_option("arena_guard") == 0 and p.get_option("arena_fill") == 0
    return g, p


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for g, p, _ in _pairs.values():
        g.close()
        p.close()
    _pairs.clear()


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_bit_equal(got, exp, what):
    assert len(got) == len(exp), what
    for i, (a, b) in enumerate(zip(got, exp)):
        if a is None and b is None:
            continue
        ba, bb = _bits(a), _bits(b)
        assert ba.shape == bb.shape, (what, i)
        if not np.array_equal(ba, bb):
            fa, fb = np.asarray(a.cpu() if hasattr(a, "cpu") else a, np.float64), np.asarray(b.cpu() if hasattr(b, "cpu") else b, np.float64)
            raise AssertionError("%s: output %d differs under the guarded, NaN-filled workspace: %d of %d values, %d NaN (plain: %d)"
                                 % (what, i, int((fa != fb).sum()), fa.size, int(np.isnan(fa).sum()), int(np.isnan(fb).sum())))


def _assert_clean(m, what):
    n, buf, off, msg = m.arena_check(detail=True)
    assert n == 0, "%s: %d guard words overwritten; %s" % (what, n, msg)


# ---- the full table: the only pass with the img and ds buffers, the past-flow decoders and flow_b ----

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("B,H,Wd", SIZES)
@pytest.mark.parametrize("which", KINDS)
def test_full_table(which, B, H, Wd, setting):
    """Model.forward on the default rule and under every kernel a user can select: F(6x6), F(4x4), F(2x2), the 1-D Winograd kernel, the
    bf16-pipe kernels, both stride-2 forms and cost-volume variants 0 / 1 / 3 / 5 / 7, with NaN on every side of every buffer."""
    x, flat = _case(which, B, H, Wd)
    g, p = _pair(which, flat, (B, H, Wd))
    opts = {} if setting == "default" else dict({"adaptive_kernels": 0}, **KERNEL_SETTINGS[setting][0])
    what = "table %s %dx%dx%d %s" % (which, B, H, Wd, setting)
    with g.options(**opts), p.options(**opts):
        got = g.forward(x)
        _assert_clean(g, what)
        exp = p.forward(x)
    assert len(got) == (25 if which == "soft" else 20)
    assert all(np.isfinite(a).all() for a in exp), what
    _assert_bit_equal(got, exp, what)


def test_forward_output_table_is_guarded():
    """With arena_guard set, every tensor of b2f_forward's output table is a guarded device buffer that starts as the NaN pattern and is
    checked before the download (shipped and generic contexts alike; the generic ones: tests/test_gpu_graph_guards.py): the kernels that
    store straight into the table -- the flow and occlusion outputs, the image warps -- write every element and nothing else, so the
    guarded context gives the plain context's bits with no word of the pattern among them."""
    for which in KINDS:
        x, flat = _case(which, 1, 192, 320)
        g, p = _pair(which, flat, (1, 192, 320))
        got = g.forward(x)
        _assert_clean(g, "output table %s" % which)
        assert not any((a.view(np.uint32) == 0x7fc0a5a5).any() for a in got), which
        _assert_bit_equal(got, p.forward(x), "output table %s" % which)


# ---- the pruned graph: eager, capture, replay ----

def _device_rounds(which, B, H, Wd, past_out, what):
    x, flat = _case(which, *((B, H, Wd) if (B, H, Wd) in SIZES else (2, 128, 192)))
    g, p = _pair(which, flat, (B, H, Wd) if (B, H, Wd) in SIZES else (2, 128, 192))
    d_in = torch.from_numpy(np.ascontiguousarray(x[:B])).cuda()
    outs = {}
    for m in (g, p):
        outs[m] = _outs(m, B, H, Wd) + ([torch.empty((B, 2, H, Wd), device="cuda")] if past_out else [])
    with g.options(use_graph=1), p.options(use_graph=1):
        for rnd, mode in enumerate(("eager", "capture", "replay")):
            for m in (g, p):
                for o in outs[m]:
                    o.fill_(float(7 + rnd))
                torch.cuda.synchronize()
                o3 = [o.data_ptr() for o in outs[m][:3]]
                m.forward_device(d_in.data_ptr(), B, H, Wd, *o3, d_past_flow=outs[m][3].data_ptr() if past_out else None)
                m.synchronize()
            _assert_clean(g, "%s %s" % (what, mode))
            assert all(bool(torch.isfinite(o).all()) for o in outs[p]), (what, mode)
            _assert_bit_equal(outs[g], outs[p], "%s %s" % (what, mode))


@pytest.mark.parametrize("B,H,Wd", SIZES + [(1, 128, 192)])
@pytest.mark.parametrize("which", KINDS)
def test_pruned_graph(which, B, H, Wd):
    """forward_device with use_graph = 1, three calls on the same pointers: the captured graph carries the guarded offsets.  The
    single-triplet sizes take the per-launch kernel rule (adaptive_kernels = -1)."""
    _device_rounds(which, B, H, Wd, False, "forward_device %s %dx%dx%d" % (which, B, H, Wd))


@pytest.mark.parametrize("B,H,Wd", SIZES)
def test_pruned_graph_with_the_past_flow(B, H, Wd):
    _device_rounds("soft", B, H, Wd, True, "forward_device_past %dx%dx%d" % (B, H, Wd))


# ---- sequence and stream ----

def _clip(seed, T, H, Wd):
    return np.random.default_rng(seed).integers(0, 256, (T, 3, H, Wd), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["unit", "u8"])
@pytest.mark.parametrize("which", KINDS)
def test_sequence(which, kind):
    T, H, Wd = 4, 128, 192
    g, p = _pair(which, _case(which, 2, 128, 192)[1], (2, 128, 192))
    by = _clip(11, T, H, Wd)
    frames = by if kind == "u8" else by.astype(np.float32) / np.float32(255)
    d = torch.from_numpy(frames).cuda()
    in_kind = back2future.IN_U8 if kind == "u8" else back2future.IN_UNIT
    outs = {m: _outs(m, T - 2, H, Wd) for m in (g, p)}
    for m in (g, p):
        m.forward_sequence_device(d.data_ptr(), T, H, Wd, *[o.data_ptr() for o in outs[m]], in_kind=in_kind)
        m.synchronize()
    what = "sequence %s %s" % (which, kind)
    _assert_clean(g, what)
    assert all(bool(torch.isfinite(o).all()) for o in outs[p]), what
    _assert_bit_equal(outs[g], outs[p], what)


@pytest.mark.parametrize("which", KINDS)
def test_stream(which):
    """Five pushes into a stream of the guarded context (its device block starts as the NaN pattern too) equal the sequence of the plain
    one; between two pushes a batch at a larger size lays the arena out anew."""
    T, H, Wd = 5, 128, 192
    g, p = _pair(which, _case(which, 2, 128, 192)[1], (2, 128, 192))
    V, big = _clip(12, T, H, Wd), _clip(13, 5, 192, 256)
    exp = p.computeFlowSequence(V, dtype=np.float32, occ_prob=True)
    exp_big = p.computeFlowBatch(big[:3], big[1:4], big[2:5], dtype=np.float32)
    with g.openStream(H, Wd) as st:
        for k in range(T):
            got = st.push(V[k], occ_prob=True)
            _assert_clean(g, "stream %s push %d" % (which, k + 1))
            assert (got is None) == (k < 2)
            if got is not None:
                _assert_bit_equal([a[0] for a in got], [b[k - 2] for b in exp], "stream %s push %d" % (which, k + 1))
            got_big = g.computeFlowBatch(big[:3], big[1:4], big[2:5], dtype=np.float32)
            _assert_clean(g, "stream %s: batch after push %d" % (which, k + 1))
            _assert_bit_equal(got_big, exp_big, "stream %s: batch after push %d" % (which, k + 1))


# ---- a warm context ----

def test_growing_shapes_match_a_fresh_unguarded_context():
    """The shapes of test_growing_shapes_match_a_fresh_context in their order, ending on the smaller one: every reallocation of the
    arena, and every pass that lays a grown arena out differently, starts from the pattern again."""
    r = np.random.default_rng(77)
    old = _guarded("random:soft:4:2.0")
    try:
        for n, H0, W0 in [(1, 64, 64), (2, 100, 180), (3, 128, 256), (4, 200, 300), (5, 264, 374), (6, 320, 448), (2, 70, 90)]:
            ims = [r.random((n, 3, H0, W0), dtype=np.float32) for _ in range(3)]
            got = old.computeFlowBatch(*ims)
            _assert_clean(old, "warm context %dx%dx%d" % (n, H0, W0))
            fresh = back2future.Model("random:soft:4:2.0")
            try:
                exp = fresh.computeFlowBatch(*ims)
            finally:
                fresh.close()
            _assert_bit_equal(got, exp, "warm context %dx%dx%d" % (n, H0, W0))
    finally:
        old.close()


# ---- the detectors detect ----

def test_selftest_reports_the_overwritten_word():
    """One guard word overwritten by a copy from the host (no kernel stores out of range): b2f_arena_check reports exactly that buffer
    and offset, and the check of a guarded op-level buffer fails with the buffer's name, side and offset."""
    x, flat = _case("soft", 1, 64, 64)
    m = _guarded("random:soft:%d:2.0" % SEED)
    try:
        m.set_weights(flat)
        assert m.arena_check() == 0                          # no pass yet: nothing laid out
        with pytest.raises(_lib.B2FError, match="no guarded plan"):
            m.guard_selftest(0)
        m.forward(x)                                         # the full table of a Soft model: img, tmp, cs[2], ...
        assert m.arena_check(detail=True)[:3] == (0, -1, 0)
        m.guard_selftest(0)
        n, buf, off, msg = m.arena_check(detail=True)
        assert (n, buf, off) == (1, 1, 3) and "after buffer 'tmp'" in msg and "0x3f800000" in msg, (n, buf, off, msg)
        m.guard_selftest(1)
        n, buf, off, msg = m.arena_check(detail=True)
        assert (n, buf, off) == (2, 0, -2) and "before buffer 'img'" in msg, (n, buf, off, msg)
        m.set_option("arena_fill", 1)                        # setting an arena option frees the arena: the next pass fills afresh
        d_in = torch.from_numpy(x).cuda()
        outs = _outs(m, 1, 64, 64)
        m.forward_device(d_in.data_ptr(), 1, 64, 64, *[o.data_ptr() for o in outs])
        assert m.arena_check() == 0
        m.guard_selftest(0)                                  # the pruned pass has no img: buffer 1 is cs[2]
        n, buf, off, msg = m.arena_check(detail=True)
        assert (n, buf, off) == (1, 1, 3) and "after buffer 'cs[2]'" in msg, (n, buf, off, msg)
        with pytest.raises(_lib.B2FError, match=r"'selftest' \(1000 floats\) overwritten: 1 words, the first one after the buffer at offset \+2 from its end"):
            m.guard_selftest(2)
        with pytest.raises(_lib.B2FError, match=r"'selftest' \(1000 floats\) overwritten: 1 words, the first one before the buffer at offset -1 from its start"):
            m.guard_selftest(3)
        # the op entries' staging scope holds 'a' (10 floats), 'b' (1000 floats) and 'c' (7 bytes): it checks what it owns, without a list
        with pytest.raises(_lib.B2FError, match=r"'b' \(1000 floats\) overwritten: 1 words, the first one after the buffer at offset \+2 from its end"):
            m.guard_selftest(4)
        with pytest.raises(_lib.B2FError, match=r"'c' \(2 floats\) overwritten: 1 words, the first one before the buffer at offset -1 from its start"):
            m.guard_selftest(5)
        with pytest.raises(_lib.B2FError):
            m.set_option("arena_guard", 100)                 # not a multiple of 64
        m.set_option("arena_guard", 0)
        m.forward_device(d_in.data_ptr(), 1, 64, 64, *[o.data_ptr() for o in outs])
        assert m.arena_check() == 0                          # no guards, nothing to report
    finally:
        m.close()
