#!/usr/bin/env python3
"""RNS inner product (include/gpuntt/rns/inner_product.cuh), timed at the shapes of DESIGN.md 3.11 against
  (a) a same-session torch device-to-device copy that moves the same number of bytes, and
  (b) the composition a caller had before: per key component, digit and limb one elementwise product launch, and one
      elementwise addition launch per further digit (operator_gpu: one modulus and one polynomial per launch, so
      C * count * M * (2 D - 1) launches; GPU_PointwiseMul would need C * D launches for the products and is C++
      only).  Timed for count = 1 and for D = 1.
Traffic of one call: D*count*M*N + D*C*M*N words read, C*count*M*N written.  One call's buffers fit the Infinity Cache
(256 MiB), so every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a
set: every timed call reads from HBM.  Per case: warm-up, then the median of --iters per-iteration HIP event pairs.
One JSON line per case.
    python tools/bench_innerproduct.py [--iters 100] [--out profiles/innerproduct_bench.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import _load_pkg  # noqa: E402
from gpu_utils import find_ntt_factors  # noqa: E402

ROTATE_BYTES = 512 << 20


def median_ms(fn, iters, warmup=10):
    """fn(i) is the i-th call: it picks its own buffer set"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(warmup + i)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--only", default=None, help="run the named case alone (rocprofv3 runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, M, D, C, count
        ("c5_keyswitch_count1", 64, 16, 8, 3, 2, 1),
        ("c5_keyswitch_count16", 64, 16, 8, 3, 2, 16),
        ("u32_keyswitch_count16", 32, 14, 8, 4, 2, 16),
        ("hadamard_count16", 64, 16, 8, 1, 1, 16),
    ]
    lines = []
    for name, bits, logn, M, D, C, count in shapes:
        if args.only and name != args.only:
            continue
        n, wsz = 1 << logn, bits // 8
        dt = torch.int64 if bits == 64 else torch.int32
        qs = [find_ntt_factors(60 if bits == 64 else 30, 3, skip=i, clear_of_top=True)[0] for i in range(M)]
        plan = g.InnerProductPlan(qs, bits)
        words = (D * count * M * n, D * C * M * n, C * count * M * n)
        traffic = sum(words) * wsz
        nsets = max(2, -(-ROTATE_BYTES // traffic) + 1)
        sets = [tuple(torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for w in words) for _ in range(nsets)]
        copies = [(torch.randint(0, 1 << 20, (traffic // (2 * wsz),), dtype=dt, device=dev),
                   torch.empty(traffic // (2 * wsz), dtype=dt, device=dev)) for _ in range(nsets)]

        def call(i):
            a, key, out = sets[i % nsets]
            plan.multiply_accumulate(a, key, out, logn, D, C, count)

        def copy(i):
            src, dst = copies[i % nsets]
            dst.copy_(src)

        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "M": M, "D": D, "C": C, "count": count,
               "traffic_bytes": traffic, "buffer_sets": nsets}
        res["copy_ms"] = median_ms(copy, args.iters)
        res["innerprod_ms"] = median_ms(call, args.iters)
        res["innerprod_TBps"] = round(traffic / (res["innerprod_ms"] * 1e-3) / 1e12, 3)
        res["copy_TBps"] = round(traffic / (res["copy_ms"] * 1e-3) / 1e12, 3)
        res["innerprod_over_copy"] = round(res["innerprod_ms"] / res["copy_ms"], 3)
        del copies
        if count == 1 or D == 1:
            # (b) timing, not a check: limb views of the same buffers, one modulus per launch
            qm = [g.Modulus(q, bits=bits) for q in qs]
            launches = C * count * M * (2 * D - 1)

            def composed(i):
                a, key, _ = sets[i % nsets]
                for c in range(C):
                    for r in range(count):
                        for m in range(M):
                            acc = None
                            for d in range(D):
                                av = a[((d * count + r) * M + m) * n:][:n]
                                kv = key[((d * C + c) * M + m) * n:][:n]
                                p = g.operator_gpu(2, av, kv, qm[m])
                                acc = p if acc is None else g.operator_gpu(0, acc, p, qm[m])

            res["composition_launches"] = launches
            res["operator_gpu_composition_ms"] = median_ms(composed, max(3, args.iters // 10), warmup=2)
            res["composition_over_innerprod"] = round(res["operator_gpu_composition_ms"] / res["innerprod_ms"], 1)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
