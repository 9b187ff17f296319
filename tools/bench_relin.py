#!/usr/bin/env python3
"""KeySwitchPlan.multiply_relinearize (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.15 against
the path a caller had before it -- the composition of the call's definition: per input three q-base
InnerProductPlan.multiply_accumulate calls (the polynomials of y in the key's place, gather copies for the cross term),
one KeySwitchPlan.apply on the top term and two modular additions (torch.where).  Before anything is timed the two
sides are checked equal on one buffer set.  Every case rotates over enough distinct buffer sets that more than 512 MiB
pass between two uses of a set: every timed call reads from HBM.  Per case: warm-up, then the median of --iters HIP event
pairs, each around --calls back-to-back calls (the figure is per call), taken --repeats times alternating the two sides,
so the spread of the baseline's own medians is recorded next to the ratio.  One JSON line per case.
    python tools/bench_relin.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/relin_bench.jsonl]"""
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


def median_ms(fn, iters, warmup=3, calls=1):
    """fn(i) is the i-th call: it picks its own buffer set.  One HIP event pair brackets `calls` consecutive calls"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (a, b) in enumerate(ev):
        a.record()
        for j in range(calls):
            fn(warmup + i * calls + j)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="calls per HIP event pair")
    ap.add_argument("--repeats", type=int, default=3, help="medians per side, alternating")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_relin.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, K, alpha, count
        ("u64_count1", 64, 16, 6, 2, 2, 1),
        ("u64_count16", 64, 16, 6, 2, 2, 16),
        ("u32_count16", 32, 14, 6, 2, 2, 16),
    ]
    lines = []
    for name, bits, logn, L, K, alpha, count in shapes:
        if args.only and name != args.only:
            continue
        M, n, wsz = L + K, 1 << logn, bits // 8
        D = -(-L // alpha)
        dt = torch.int64 if bits == 64 else torch.int32
        npdt = g.np_dtype(bits)
        cases = []
        fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
        for i in range(M):
            f = find_ntt_factors(59 if bits == 64 else 29, logn, skip=i, clear_of_top=True)
            prm = g.NTTParameters(logn, g.X_N_plus, bits, f)
            cases.append(prm)
            fwd[i * n:i * n + prm.root_of_unity_size] = prm.forward_table_device_order
            inv[i * n:i * n + prm.root_of_unity_size] = prm.inverse_table_device_order
        qs = [p.modulus.value for p in cases]
        ninv = [p.n_inv for p in cases]
        d_fwd, d_inv = g.to_device(fwd), g.to_device(inv)
        plan = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, d_fwd, d_inv, ninv, g.X_N_plus,
                               batch_hint=D * count * M, bits=bits)
        inner_q = g.InnerProductPlan(qs[:L], bits=bits)
        qt = g.to_device(np.array(qs[:L], dtype=npdt)).view(1, 1, L, 1)
        # the key is shared by every buffer set (what an evaluator keeps resident)
        key = torch.randint(0, min(qs), (D * 2 * M * n,), dtype=dt, device=dev)
        ct = 2 * count * L * n
        words = dict(x=ct, y=ct, out=ct, d=3 * count * L * n, k=ct, ga=2 * L * n, gk=2 * L * n)
        sbytes = plan.scratch_bytes(count, 2)
        per_set = sum(words.values()) * wsz + sbytes
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["scratch"] = torch.zeros(sbytes, dtype=torch.uint8, device=dev)

        def fused(i, out=None):
            s = sets[i % nsets]
            plan.multiply_relinearize(s["x"], s["y"], key, s["out"] if out is None else out, count, True, s["scratch"])

        def baseline(i, out=None):
            s = sets[i % nsets]
            x, y, d = s["x"].view(2, count, L * n), s["y"].view(2, count, L * n), s["d"].view(3, count, L * n)
            ga, gk = s["ga"].view(2, L * n), s["gk"].view(2, L * n)
            for r in range(count):  # the key operand is shared by all inputs: one call per input and term
                inner_q.multiply_accumulate(x[0, r], y[0, r], d[0, r], logn, 1, 1, 1)
                ga[0].copy_(x[0, r]), ga[1].copy_(x[1, r]), gk[0].copy_(y[1, r]), gk[1].copy_(y[0, r])
                inner_q.multiply_accumulate(s["ga"], s["gk"], d[1, r], logn, 2, 1, 1)
                inner_q.multiply_accumulate(x[1, r], y[1, r], d[2, r], logn, 1, 1, 1)
            plan.apply(d[2].reshape(-1), key, s["k"], count, 2, True, True, s["scratch"])
            t = s["k"].view(2, count, L, n) + d[:2].view(2, count, L, n)
            torch.where(t >= qt, t - qt, t, out=(s["out"] if out is None else out).view(2, count, L, n))

        a, b = torch.empty(ct, dtype=dt, device=dev), torch.empty(ct, dtype=dt, device=dev)
        fused(0, a), baseline(0, b)
        torch.cuda.synchronize()
        same = bool(torch.equal(a, b))
        del a, b
        unit = L * n * wsz * count  # bytes of count L N words
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "count": count,
               "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls,
               "matches_the_composition": same,
               # beyond apply's own traffic, a count: x1, y1 -> d2, then four input words / the three
               # products with their outputs, the gathers, and the two additions
               "extra_bytes_fused": 8 * unit, "extra_bytes_composition": 25 * unit,
               "launches_before_the_switch": {"fused": 1, "composition": 3 * count}}
        mine, theirs = [], []
        for _ in range(args.repeats):  # alternating, so both sides see the same neighbours on the machine
            theirs.append(median_ms(baseline, args.iters, calls=args.calls))
            mine.append(median_ms(fused, args.iters, calls=args.calls))
        res["multiply_relinearize_ms"] = [round(v, 5) for v in mine]
        res["composition_ms"] = [round(v, 5) for v in theirs]
        res["fused_over_composition"] = round(float(np.median(mine)) / float(np.median(theirs)), 3)
        res["baseline_spread"] = round((max(theirs) - min(theirs)) / float(np.median(theirs)), 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan, key, inner_q
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
