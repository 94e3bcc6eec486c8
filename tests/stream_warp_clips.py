"""The clips of the stream warp tests (tests/test_gpu_stream_warp.py, tests/test_stream_warp_cpu.py) and what makes them fit for
the job: a push that samples the wrong ring slot must not be able to pass, so the three frames of every triplet have to be different
enough that exchanging two of them shows in the host definition of the warp (ops.flow_warp(model=None)).  The frames are independent
uniform noise: two of them agree in a sample with probability 1 / 256 (bytes) or practically never (floats)."""
import numpy as np

from back2future_amd import ops

T = 7                              # every ring slot is written at least twice
SIZES = [(128, 192), (136, 200)]   # a /64 size (the frame slots hold the caller's frames) and a rescaled one (the raw ring does)
SEEDS = (21, 22)                   # camera 0 / the first clip, camera 1 / the clip after a reset


def clip(seed, H0, W0, dtype, frames=T):
    """T x 3 x H0 x W0 frames of `dtype` (np.uint8, or np.float32 in [0, 1))"""
    r = np.random.default_rng(1000 * seed + H0 + W0)
    if np.dtype(dtype) == np.uint8:
        return r.integers(0, 256, (frames, 3, H0, W0), dtype=np.uint8)
    return r.random((frames, 3, H0, W0), dtype=np.float32)


def probe_flow(seed, H0, W0):
    """(flow, occ_prob), 1 x 2 x H0 x W0 float32 each, for the host definition: a raw flow of up to +-0.25 (5 pixels at flow_scale 20) and
    probabilities in [0, 1)"""
    r = np.random.default_rng(seed)
    return ((r.random((1, 2, H0, W0), dtype=np.float32) - np.float32(0.5)) * np.float32(0.5)), r.random((1, 2, H0, W0), dtype=np.float32)


def differing_pixels(a, b):
    """share of the pixels of two 3 x H x W frames that differ in at least one channel"""
    return float((a != b).any(axis=0).mean())


def host_warp(V, k, flow, prob):
    """the host definition on the triplet (k - 2, k - 1, k) of clip V, frames given as (past, reference, future)"""
    return ops.flow_warp(flow, V[k - 2][None], V[k - 1][None], V[k][None], occ_prob=prob, model=None)


def exchange_changes(V, k, flow, prob, swap):
    """(share of warped samples that change, photo words that change) when two frames of the triplet (k - 2, k - 1, k) trade places in
    the host definition; swap: a pair of positions in (past, reference, future)"""
    tri = [V[k - 2][None], V[k - 1][None], V[k][None]]
    w0, p0 = ops.flow_warp(flow, *tri, occ_prob=prob, model=None)
    tri[swap[0]], tri[swap[1]] = tri[swap[1]], tri[swap[0]]
    w1, p1 = ops.flow_warp(flow, *tri, occ_prob=prob, model=None)
    return float((w0 != w1).mean()), int((p0 != p1).sum())
