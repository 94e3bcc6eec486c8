"""The FIRST call of every launcher, met by four threads at once.

A launcher sets its kernel's dynamic-LDS attribute and reads the CU count on its first call per device (LdsOnce, device_cu_count of
csrc/b2f_internal.h).  b2f_multi runs one worker thread per replica, so with GPU 0 listed four times four threads make that first
call together.  It happens once per process, and the suite's own process has long warmed every kernel, hence a fresh child whose
first GPU work is the multi batch; only afterwards does it create the single context that the results must equal bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_first_launches_from_four_threads_match_one_context():
    """4 byte triplets at 512 x 512 on four replicas of GPU 0: the smallest square frame whose level-3 map (128 x 128 = 16 384 pixels)
    reaches wino6_min_pixels, so the F(6x6), F(4x4), F(2x2), stride-2, head and cost-volume launchers all run, each for the first
    time, on four threads.  Flow and both masks equal those of one context, created afterwards from the same weights."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import numpy as np\n"
        "from back2future_amd import back2future\n"
        "r = np.random.default_rng(41)\n"
        "ims = [r.integers(0, 256, (4, 3, 512, 512), dtype=np.uint8) for _ in range(3)]\n"
        "mm = back2future.MultiModel('random:hard:3:2.0', n_gpus=4, devices=[0] * 4)\n"
        "assert mm.n_gpus == 4 and mm.devices == [0] * 4\n"
        "got = mm.computeFlowBatch(*ims)\n"          # the process's first GPU work
        "ref = back2future.Model('random:hard:3:2.0')\n"
        "exp = ref.computeFlowBatch(*ims)\n"
        "assert len(got) == 3 and len(exp) == 3\n"
        "assert np.abs(exp[0]).max() > 0 and np.isfinite(exp[0]).all()\n"
        "for name, a, b in zip(('flow', 'fwd mask', 'bwd mask'), got, exp):\n"
        "    assert a.shape == b.shape and a.shape[0] == 4, (name, a.shape, b.shape)\n"
        "    assert np.array_equal(a, b), name\n"
        "mm.close()\n"
        "ref.close()\n"
        "print('ok')\n")
    env = dict(os.environ, B2F_MULTI_TRANSPORT="peer", B2F_MULTI_ALLOW_DUPLICATE="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
