#!/usr/bin/env python3
"""RNS base conversion (include/gpuntt/rns/base_conversion.cuh), timed at the shapes of DESIGN.md 3.10: ModUp, ModDown
(convert-and-divide, centred), rescale, a 32-bit shape and a launch-bound one, against
  (a) a same-session torch device-to-device copy of the same bytes, and
  (b) for the 8 -> 24 ModUp: what a caller could do before, the L * K operator_gpu mult / add composition.
Traffic of one call: (L + K) * N * count * sizeof(T), plus K * N * count * sizeof(T) for c.  Per case: warm-up, then the
median of --iters per-iteration HIP event pairs.  One JSON line per case.  --ksplit 1,2,4,8 also times the forced
split of the outputs over that many workgroups per column tile (test hook baseconv_ksplit).
    python tools/bench_baseconv.py [--iters 100] [--ksplit 1,2,4,8] [--out profiles/baseconv_bench.jsonl]"""
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

PEAK_BPS = 8e12  # MI355X HBM3E, datasheet


def median_ms(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--ksplit", default="")
    ap.add_argument("--only", default=None, help="run the named case alone (rocprofv3 runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, L, K, logn, count, divide, mode
        ("modup_4_28", 64, 4, 28, 16, 16, False, g.APPROXIMATE),
        ("modup_8_24", 64, 8, 24, 16, 16, False, g.APPROXIMATE),
        ("moddown_8_24", 64, 8, 24, 16, 16, True, g.CENTRED),
        ("rescale_1_31", 64, 1, 31, 16, 16, True, g.CENTRED),
        ("u32_8_8", 32, 8, 8, 14, 64, False, g.APPROXIMATE),
        ("launch_bound_3_5", 64, 3, 5, 12, 1, False, g.APPROXIMATE),
    ]
    splits = [int(s) for s in args.ksplit.split(",") if s]
    lines = []
    for name, bits, L, K, logn, count, divide, mode in shapes:
        if args.only and name != args.only:
            continue
        n = 1 << logn
        dt = torch.int64 if bits == 64 else torch.int32
        wsz = bits // 8
        ms = [find_ntt_factors(60 if bits == 64 else 30, 3, skip=i, clear_of_top=True)[0] for i in range(L + K)]
        qs, ps = ms[:L], ms[L:]
        plan = g.BaseConvPlan(qs, ps, bits)
        x = torch.randint(0, min(qs), (count * L * n,), dtype=dt, device=dev)
        c = torch.randint(0, min(ps), (count * K * n,), dtype=dt, device=dev)
        out = torch.empty_like(c)
        traffic = (L + K + (K if divide else 0)) * n * count * wsz
        src = torch.randint(0, 1 << 20, (traffic // (2 * wsz),), dtype=dt, device=dev)
        dst = torch.empty_like(src)

        def call():
            if divide:
                plan.convert_and_divide(x, c, out, logn, count, mode)
            else:
                plan.convert(x, out, logn, count, mode)

        res = {"case": name, "dtype": "u%d" % bits, "L": L, "K": K, "logN": logn, "count": count,
               "divide": divide, "mode": "centred" if mode == g.CENTRED else "approximate", "traffic_bytes": traffic}
        res["copy_ms"] = median_ms(lambda: dst.copy_(src), args.iters)
        res["baseconv_ms"] = median_ms(call, args.iters)
        for s in splits:
            g.set_test_hook("baseconv_ksplit", s)
            res["baseconv_ms_ksplit_%d" % s] = median_ms(call, args.iters)
        g.set_test_hook("baseconv_ksplit", 0)
        res["baseconv_TBps"] = round(traffic / (res["baseconv_ms"] * 1e-3) / 1e12, 3)
        res["copy_TBps"] = round(traffic / (res["copy_ms"] * 1e-3) / 1e12, 3)
        res["baseconv_over_copy"] = round(res["baseconv_ms"] / res["copy_ms"], 3)
        res["mac_per_coefficient"] = L * K
        if name == "modup_8_24":
            # (b) the composition a caller had: y_i = x_i * w_i mod q_i (L launches), then for every output limb
            # L mults and L - 1 adds mod p_j, one launch and one pass over HBM each.  The limbs are views of the
            # buffers; the inputs are reduced mod p_j by the mult itself only when q_i < p_j, which a real caller
            # would have to handle too -- this is timing, not a check
            qm, pm = [g.Modulus(q, bits=bits) for q in qs], [g.Modulus(p, bits=bits) for p in ps]
            xl = [x[i * n * count:(i + 1) * n * count] for i in range(L)]
            w = [torch.randint(0, min(ps), (n * count,), dtype=dt, device=dev) for _ in range(L)]

            def composed():
                y = [g.operator_gpu(2, xl[i], w[i], qm[i]) for i in range(L)]
                for j in range(K):
                    acc = g.operator_gpu(2, y[0], w[0], pm[j])
                    for i in range(1, L):
                        acc = g.operator_gpu(0, acc, g.operator_gpu(2, y[i], w[i], pm[j]), pm[j])

            res["operator_gpu_composition_ms"] = median_ms(composed, max(3, args.iters // 10), warmup=2)
            res["composition_over_baseconv"] = round(res["operator_gpu_composition_ms"] / res["baseconv_ms"], 1)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del x, c, out, src, dst, plan
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
