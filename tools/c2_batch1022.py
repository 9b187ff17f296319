#!/usr/bin/env python3
"""The C2 call (forward u64 Merge NTT, N = 2^16, X^N - 1, in place, drop-in) at batch 1022 -- no multiple of 4, so the
10-stage last pass runs on the one-polynomial tile: 400 timed calls after 50, one JSON line in bench.py's form
(`ms_per_step`, `batch_check.bit_exact` from five polynomials against the oracle).  A line of tools/ab_lib.py ... c2."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from __graft_entry__ import _load_pkg  # noqa: E402

g = _load_pkg()
g.load_library()
from oracle import oracle as O  # noqa: E402

LOGN, BATCH, STEPS, WARMUP = 16, 1022, 400, 50
N = 1 << LOGN
P = O.Port(64)
prm = g.NTTParameters(LOGN, g.X_N_minus, 64)
oprm = P.merge_params(LOGN, O.X_N_minus)
x = P.splitmix(0x5EED, 0, BATCH * N, prm.modulus.value)
d = g.to_device(x)
table = g.to_device(prm.forward_table_device_order)
cfg = g.ntt_configuration(n_power=LOGN, reduction_poly=g.X_N_minus)


def call():
    g.GPU_NTT_Inplace(d, table, prm.modulus, cfg, BATCH)


call()
torch.cuda.synchronize()
got = g.to_host(d)
exact = all(np.array_equal(got[p * N:(p + 1) * N], P.merge_ntt(x[p * N:(p + 1) * N], oprm)) for p in (0, 1, 511, 1020, 1021))
for _ in range(WARMUP):
    call()
torch.cuda.synchronize()
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
start.record()
for _ in range(STEPS):
    call()
stop.record()
torch.cuda.synchronize()
print(json.dumps({"ms_per_step": start.elapsed_time(stop) / STEPS, "batch_check": {"bit_exact": bool(exact)}}))
