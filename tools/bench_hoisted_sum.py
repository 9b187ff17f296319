#!/usr/bin/env python3
"""KeySwitchPlan.rotate_hoisted_sum (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.14 against the
path a caller had before it: rotate_hoisted(output_ntt=True) over the G elements, then ONE q-base
InnerProductPlan.multiply_accumulate over the G outputs (the G stacks as digits, q-base weights as the key).  The two
do not produce the same words -- the older path rounds G times, the new call once (key_switch.cuh) -- so before anything
is timed the tool checks the new call against its own definition, tests/hoisted_sum_utils.composition_sum, once per shape.
Every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set: every timed
call reads from HBM.  Per case: warm-up, then the median of --iters HIP event pairs, each around --calls back-to-back
calls (the figure is per call), taken --repeats times alternating the two sides, so the spread of the baseline's own
medians is recorded next to the ratio.  One JSON line per case.
    python tools/bench_hoisted_sum.py [--iters 30] [--calls 5] [--repeats 3] [--out profiles/hoisted_sum_bench.jsonl]"""
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
from hoisted_sum_utils import composition_sum  # noqa: E402

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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5, help="calls per HIP event pair")
    ap.add_argument("--repeats", type=int, default=3, help="medians per side, alternating")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hoisted_sum.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, K, alpha, G, count
        ("u64_count1", 64, 16, 6, 2, 2, 8, 1),
        ("u64_count16", 64, 16, 6, 2, 2, 8, 16),
        ("u32_count16", 32, 14, 6, 2, 2, 8, 16),
    ]
    lines = []
    for name, bits, logn, L, K, alpha, G, count in shapes:
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
                               batch_hint=G * 2 * count * M, bits=bits)
        inner_q = g.InnerProductPlan(qs[:L], bits=bits)
        elts = [g.galois_element_for_rotation(s + 1, logn) for s in range(G)]
        # keys and weights are shared by every buffer set (what a linear transform keeps resident): G keys of D 2 M N
        # words, G full-base weights of M N words for the new call, their q-limbs as a key T[G][1][L][N] for the baseline
        keys = [torch.randint(0, min(qs), (D * 2 * M * n,), dtype=dt, device=dev) for _ in range(G)]
        weights = [torch.randint(0, min(qs), (M * n,), dtype=dt, device=dev) for _ in range(G)]
        weights_q = torch.cat([w[:L * n] for w in weights])
        words = dict(a=D * count * M * n, c0=count * L * n, out=2 * count * L * n, rot=G * 2 * count * L * n)
        sum_bytes, hoist_bytes = plan.hoisted_sum_scratch_bytes(count), plan.hoisted_scratch_bytes(count, G)
        per_set = sum(words.values()) * wsz + sum_bytes + hoist_bytes
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["sum"] = torch.zeros(sum_bytes, dtype=torch.uint8, device=dev)
            s["hoist"] = torch.zeros(hoist_bytes, dtype=torch.uint8, device=dev)

        def summed(i, out=None):
            s = sets[i % nsets]
            plan.rotate_hoisted_sum(s["a"], s["c0"], keys, elts, weights, s["out"] if out is None else out, count, True,
                                    s["sum"])

        def baseline(i):
            s = sets[i % nsets]
            plan.rotate_hoisted(s["a"], s["c0"], keys, elts, s["rot"], count, True, s["hoist"])
            inner_q.multiply_accumulate(s["rot"], weights_q, s["out"], logn, G, 1, 2 * count)

        st = dict(moduli=qs, poly=g.X_N_plus, mods=g.modulus_array_to_device([p.modulus for p in cases], bits),
                  fwd=d_fwd, inv=d_inv, d_ninv=g.to_device(np.array(ninv, dtype=npdt)))
        check = torch.empty(words["out"], dtype=dt, device=dev)
        summed(0, check)
        torch.cuda.synchronize()
        same = bool(torch.equal(check, composition_sum(g, plan, st, sets[0]["a"], sets[0]["c0"], keys, elts, weights,
                                                       count, True)))
        del check
        unit = M * n * wsz * count  # bytes of M N words per input
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "G": G, "count": count,
               "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls,
               "matches_its_definition": same,
               # the inner-product kernels alone, a count: a per element, keys, weights, acc / a once, keys, acc per element
               "inner_product_step_bytes_sum": (G * D + 2 * G * D + G + 2) * unit,
               "inner_product_step_bytes_rotations": (D + 2 * G * D + 2 * G) * unit,
               "stacks_through_intt_moddown_ntt": {"sum": 2 * count, "rotations": G * 2 * count},
               "hoist_sum_chunk_log2": g.keyswitch_hoist_sum_chunk(bits, D, logn),
               "hoist_chunk_log2": g.keyswitch_hoist_chunk(bits, D, logn)}
        mine, theirs = [], []
        for _ in range(args.repeats):  # alternating, so both sides see the same neighbours on the machine
            theirs.append(median_ms(baseline, args.iters, calls=args.calls))
            mine.append(median_ms(summed, args.iters, calls=args.calls))
        res["hoisted_sum_ms"] = [round(v, 5) for v in mine]
        res["rotations_then_product_ms"] = [round(v, 5) for v in theirs]
        res["sum_over_baseline"] = round(float(np.median(mine)) / float(np.median(theirs)), 3)
        res["baseline_spread"] = round((max(theirs) - min(theirs)) / float(np.median(theirs)), 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan, keys, weights, weights_q, inner_q
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
