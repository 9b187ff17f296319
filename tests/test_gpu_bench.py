"""bench.py --dump-outputs on the MI355X: the arrays a caller of the timed path receives after its last step, the same
from run to run for the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """Two plain runs of the headline config with the same arguments dump the same arrays, and the dump is what the timed
    path computed: after the out-of-place first call, W warm-up and K timed in-place steps, every sampled coefficient is
    that of 1 + W + K forward transforms of the seeded input by the CPU oracle (first and last sampled polynomial)."""
    import bench
    steps, warmup = 3, 1
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", str(warmup), "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and lines[0]["steps"] == steps and lines[0]["ms_per_step"] > 0
        assert os.listdir(out) == ["output.npy"]
        dumps.append(np.load(out / "output.npy"))
    a, b = dumps
    assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2 and a.nbytes <= 64 << 20
    assert np.array_equal(a, b)

    cfg = bench.CONFIGS["c2"]
    n = 1 << cfg["logn"]
    idx = bench.dump_index(cfg["batch"] * n)
    assert idx is not None and idx.size == a.shape[0]
    words = a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))
    P = O.Port(64)
    prm = P.merge_params(cfg["logn"], O.X_N_minus)
    for p in (int(idx[0]) // n, int(idx[-1]) // n):
        y = bench.splitmix64_mod(0x5EED0002, n, prm["mod"][0], offset=p * n)  # build_case's c2 input, rank 0
        for _ in range(1 + warmup + steps):
            y = P.merge_ntt(y, prm)
        sel = idx // n == p
        assert sel.any() and np.array_equal(words[sel], y[idx[sel] % n]), p
