#!/usr/bin/env python3
"""KeySwitchPlan.multiply_relinearize_sum (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.16
against what a caller had before it: T calls of multiply_relinearize into T buffers plus T - 1 modular additions
(torch.where) over both components.  At T = 1 the baseline is multiply_relinearize alone: what the run-time term loop
costs.  Before anything is timed the new call is checked against its definition, composition_relin_sum of
tests/relin_sum_utils.py (the baseline is NOT word-equal to it: it rounds T times).  The method is tools/bench_relin.py's:
every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set, so every
timed call reads from HBM; per case warm-up, then the median of --iters HIP event pairs, each around --calls
back-to-back calls (the figure is per call), taken --repeats times alternating the two sides, so the spread of the
baseline's own medians is recorded next to the ratio.  One JSON line per case and T.
    python tools/bench_relin_sum.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/relin_sum_bench.jsonl]"""
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
from relin_sum_utils import composition_relin_sum  # noqa: E402

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
    ap.add_argument("--terms", default="1,2,4,8", help="the values of T")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_relin_sum.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, K, alpha, count
        ("u64_count1", 64, 16, 6, 2, 2, 1),
        ("u64_count16", 64, 16, 6, 2, 2, 16),
        ("u32_count16", 32, 14, 6, 2, 2, 16),
    ]
    terms = sorted(int(t) for t in args.terms.split(","))
    tmax = terms[-1]
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
        qt = g.to_device(np.array(qs[:L], dtype=npdt)).view(1, 1, L, 1)
        st = dict(moduli=qs, poly=g.X_N_plus)  # what composition_relin_sum reads with output_ntt
        # the key is shared by every buffer set (what an evaluator keeps resident)
        key = torch.randint(0, min(qs), (D * 2 * M * n,), dtype=dt, device=dev)
        ct = 2 * count * L * n
        sbytes = plan.scratch_bytes(count, 2)
        # sets are sized for the largest T and counted for the smallest: every T rotates through more than ROTATE_BYTES
        nsets = max(2, -(-ROTATE_BYTES // (3 * ct * wsz + sbytes)) + 1)

        def operand():
            return torch.randint(0, min(qs), (ct,), dtype=dt, device=dev)
        sets = [dict(x=[operand() for _ in range(tmax)], y=[operand() for _ in range(tmax)],
                     part=[operand() for _ in range(tmax)], out=operand(),
                     scratch=torch.zeros(sbytes, dtype=torch.uint8, device=dev)) for _ in range(nsets)]
        for T in terms:
            def fused(i, out=None):
                s = sets[i % nsets]
                plan.multiply_relinearize_sum(s["x"][:T], s["y"][:T], key, s["out"] if out is None else out, count, True,
                                              s["scratch"])

            def baseline(i):
                s = sets[i % nsets]
                for t in range(T):
                    plan.multiply_relinearize(s["x"][t], s["y"][t], key, s["part"][t], count, True, s["scratch"])
                acc = s["part"][0].view(2, count, L, n)
                for t in range(1, T):  # both below q < 2^(W-2): no wrap in the signed type
                    u = acc + s["part"][t].view(2, count, L, n)
                    if t == T - 1:
                        torch.where(u >= qt, u - qt, u, out=s["out"].view(2, count, L, n))
                    else:
                        acc = torch.where(u >= qt, u - qt, u)

            a = torch.empty(ct, dtype=dt, device=dev)
            fused(0, a)
            torch.cuda.synchronize()
            same = bool(torch.equal(a, composition_relin_sum(g, plan, st, sets[0]["x"][:T], sets[0]["y"][:T], key, count,
                                                             True)))
            del a
            unit = L * n * wsz * count  # bytes of count L N words
            res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "count": count,
                   "terms": T, "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls,
                   "matches_the_composition": same,
                   # beyond apply's own traffic, a count: 2 T reads and a write in tensor_top_sum, 4 T
                   # reads in inner_product_tensor_sum
                   "extra_bytes_sum": (6 * T + 1) * unit, "key_switches": {"sum": 1, "baseline": T}}
            mine, theirs = [], []
            for _ in range(args.repeats):  # alternating, so both sides see the same neighbours on the machine
                theirs.append(median_ms(baseline, args.iters, calls=args.calls))
                mine.append(median_ms(fused, args.iters, calls=args.calls))
            res["multiply_relinearize_sum_ms"] = [round(v, 5) for v in mine]
            res["baseline_ms"] = [round(v, 5) for v in theirs]
            res["sum_over_baseline"] = round(float(np.median(mine)) / float(np.median(theirs)), 3)
            res["baseline_spread"] = round((max(theirs) - min(theirs)) / float(np.median(theirs)), 3)
            res["below_the_baseline_by_more_than_its_spread"] = bool(
                float(np.median(theirs)) - float(np.median(mine)) > max(theirs) - min(theirs))
            print(json.dumps(res), flush=True)
            lines.append(res)
        del sets, plan, key
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
