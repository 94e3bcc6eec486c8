"""The models of the layer tests: the Hard / Soft model with the normal weights the op tests draw, opened under one of the option sets
that name a conv kernel, with profile rows per layer shape on.  Helper, no test (tests/test_gpu_in_place.py, tests/test_gpu_conv_float64.py);
each test module keeps and closes the contexts it opens."""
import functools

import numpy as np

from back2future_amd import back2future, weights as W

BIG = 1 << 30

# option sets; every one also gets adaptive_kernels = 0 unless it sets that option
SETTINGS = {
    "default": {"adaptive_kernels": -1},
    "f4x4": {"wino4_min_pixels": 0, "wino6": 0},
    "f6x6": {"wino4_min_pixels": 0, "wino6": 1, "wino6_min_pixels": 0},
    "wino1d-1": {"wino4_min_pixels": 0, "wino6": 0, "wino1d": 1},
    "wino1d-2": {"wino4_min_pixels": 0, "wino6": 0, "wino1d": 2},
    "bf16-wide": {"wino4_min_pixels": 0, "bf16_conv": 3, "bf16_conv_min_pixels": 0},
    "f2x2-split": {"wino4_min_pixels": BIG, "wino_split_pixels": BIG},
    "adaptive": {"adaptive_kernels": 1},
    "bf16_conv-0": {"bf16_conv": 0},
    "s2_loader-0": {"s2_loader": 0},
    "s2_loader-2": {"s2_loader": 2},
    "s2_tile_groups-0": {"s2_loader": 2, "s2_tile_groups": 0},
    "s2_tiles_per_block-2": {"bf16_conv": 0, "s2_tiles_per_block": 2},
}

@functools.lru_cache(maxsize=None)
def flat(which):
    """normal weights of variance 1 / (9 Ci) per layer, normal bias: what the op tests draw"""
    past = which == "soft"
    lay, total = W.layout(past)
    r = np.random.default_rng(71 + past)
    flat = np.empty(total, np.float32)
    for name, shape, off in lay:
        n = int(np.prod(shape))
        if name.endswith(".w"):
            flat[off:off + n] = (r.standard_normal(n, dtype=np.float32) / np.sqrt(9 * shape[1])).astype(np.float32)
        else:
            flat[off:off + n] = r.standard_normal(n, dtype=np.float32)
    return flat


def open_model(which, setting):
    m = back2future.Model("random:%s:5:2.0" % which)
    m.set_weights(flat(which))
    opts = dict({"adaptive_kernels": 0}, **SETTINGS[setting])
    for k, v in dict(opts, profile=1, profile_layers=1).items():
        m.set_option(k, v)
    return m


def name(kind, level, idx):
    return ("feat%d.conv%d" % (level, idx)) if kind == "feat" else "l%d.%s.conv%d" % (level, kind, idx)
