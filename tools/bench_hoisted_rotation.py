#!/usr/bin/env python3
"""KeySwitchPlan.rotate_hoisted (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.13 against the
composition it is defined by, built here from the calls that existed before it: one GPU_Automorphism_NTT of the digits
and one of c0 for all G elements (the hoisted form of that call), then per element switch_digits and the addition of the
rotated c0 to component 0 (torch: add, compare, select).  Both produce the same words; the tool checks that once per
shape before it times anything.
Every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set: every timed
call reads from HBM.  Per case: warm-up, then the median of --iters HIP event pairs, each around --calls back-to-back
calls (the figure is per call), taken --repeats times alternating the two sides, so the spread of the composition's own
medians is recorded next to the ratio.  One JSON line per case.
    python tools/bench_hoisted_rotation.py [--iters 30] [--calls 5] [--repeats 3] [--out profiles/hoisted_rotation_bench.jsonl]"""
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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5, help="calls per HIP event pair")
    ap.add_argument("--repeats", type=int, default=3, help="medians per side, alternating")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hoisted_rotation.py needs a GPU: nothing is measured without one")
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
        elts = [g.galois_element_for_rotation(s + 1, logn) for s in range(G)]
        qt = torch.tensor(qs[:L], dtype=dt, device=dev).view(1, L, 1)
        # the keys are shared by every buffer set (G keys of D 2 M N words: what a linear transform keeps resident);
        # a, c0, out and the scratches rotate
        keys = [torch.randint(0, min(qs), (D * 2 * M * n,), dtype=dt, device=dev) for _ in range(G)]
        words = dict(a=D * count * M * n, c0=count * L * n, out=G * 2 * count * L * n,
                     a_rot=G * D * count * M * n, c0_rot=G * count * L * n)
        hoist_bytes = plan.hoisted_scratch_bytes(count, G)
        per_set = sum(words.values()) * wsz + hoist_bytes
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["hoist"] = torch.zeros(hoist_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device=dev)

        def hoisted(i, out=None):
            s = sets[i % nsets]
            plan.rotate_hoisted(s["a"], s["c0"], keys, elts, s["out"] if out is None else out, count, True, s["hoist"])

        def composed(i, out=None):
            s = sets[i % nsets]
            o = (s["out"] if out is None else out).view(G, 2, count, L, n)
            g.GPU_Automorphism_NTT(s["a"], s["a_rot"], elts, logn, g.X_N_plus, D * count * M)
            g.GPU_Automorphism_NTT(s["c0"], s["c0_rot"], elts, logn, g.X_N_plus, count * L)
            a_rot, c0_rot = s["a_rot"].view(G, -1), s["c0_rot"].view(G, count, L, n)
            for e in range(G):
                plan.switch_digits(a_rot[e], keys[e], o[e].view(-1), count, 2, True, scratch)
                t = o[e, 0] + c0_rot[e]
                o[e, 0] = torch.where(t >= qt, t - qt, t)

        check = [torch.empty(words["out"], dtype=dt, device=dev) for _ in range(2)]
        hoisted(0, check[0]), composed(0, check[1])
        torch.cuda.synchronize()
        same = bool(torch.equal(check[0], check[1]))
        del check
        col = count * n * wsz  # bytes of one limb of every input
        # the inner-product step alone, in bytes: a and c0 read once, G keys read once per input, acc written once
        ip_fused = (D * M + L) * col + G * D * 2 * M * n * wsz * count + G * 2 * M * col
        # the recipe: permuted digits and c0 written and read back, then the same key and acc traffic, then two more
        # passes over component 0 for the c0 addition
        ip_recipe = (D * M + L) * col * (1 + 2 * G) + G * D * 2 * M * n * wsz * count + G * 2 * M * col + 2 * G * L * col
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "G": G, "count": count,
               "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls, "same_words": same,
               "inner_product_step_bytes_fused": ip_fused, "inner_product_step_bytes_recipe": ip_recipe,
               "hoist_chunk_log2": g.keyswitch_hoist_chunk(bits, D, logn)}
        mine, theirs = [], []
        for _ in range(args.repeats):  # alternating, so both sides see the same neighbours on the machine
            theirs.append(median_ms(composed, args.iters, calls=args.calls))
            mine.append(median_ms(hoisted, args.iters, calls=args.calls))
        res["hoisted_ms"] = [round(v, 5) for v in mine]
        res["composition_ms"] = [round(v, 5) for v in theirs]
        res["hoisted_over_composition"] = round(float(np.median(mine)) / float(np.median(theirs)), 3)
        res["composition_spread"] = round((max(theirs) - min(theirs)) / float(np.median(theirs)), 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan, keys, scratch
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
