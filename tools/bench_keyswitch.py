#!/usr/bin/env python3
"""Hybrid key switching (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.12: mod_up, mod_down
and apply, each against
  (a) the composition of existing public calls it replaces, built here: per digit a BaseConvPlan over a gathered staging
      buffer with one device copy per polynomial in and out (ModUp), one convert_and_divide per stack (ModDown), and for
      apply those two around the drop-in GPU_NTT / InnerProductPlan / GPU_INTT calls, and
  (b) a same-session torch device-to-device copy of the call's algorithmic bytes (mod_up: L read + D M written per
      column; mod_down: M read + L written; apply: the sum over its steps).
Every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set: every timed
call reads from HBM.  Per case: warm-up, then the median of --iters HIP event pairs, each around --calls back-to-back
calls of the plan or the copy (the figure is per call; the composition, milliseconds long, is timed one call per
pair).  One JSON line per case.
    python tools/bench_keyswitch.py [--iters 50] [--calls 20] [--out profiles/keyswitch_bench.jsonl]"""
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


def median_ms(fn, iters, warmup=5, calls=1):
    """fn(i) is the i-th call: it picks its own buffer set.  One HIP event pair brackets `calls` consecutive calls and
    the figure is the pair's time over `calls`: a call of 10 microseconds is not timed through one event pair of its own"""
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20, help="plan and copy calls per HIP event pair")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, K, alpha, C, count
        ("c5_count1", 64, 16, 6, 2, 2, 2, 1),
        ("c5_count16", 64, 16, 6, 2, 2, 2, 16),
        ("u32_count16", 32, 14, 6, 2, 2, 2, 16),
    ]
    lines = []
    for name, bits, logn, L, K, alpha, C, count in shapes:
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
        d_mods = g.modulus_array_to_device([p.modulus for p in cases], bits)
        d_ninv = g.to_device(np.array(ninv, dtype=npdt))
        plan = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, d_fwd, d_inv, ninv, g.X_N_plus,
                               batch_hint=D * count * M, bits=bits)
        inner = g.InnerProductPlan(qs, bits)
        parts = [list(range(d * alpha, min((d + 1) * alpha, L))) for d in range(D)]
        ups = [g.BaseConvPlan([qs[i] for i in S], [qs[m] for m in range(M) if m not in S], bits) for S in parts]
        down = g.BaseConvPlan(qs[L:], qs[:L], bits)
        words = dict(c=count * L * n, a=D * count * M * n, key=D * C * M * n, acc=C * count * M * n,
                     out=C * count * L * n)
        per_set = sum(words.values()) * wsz
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        scratch = torch.zeros(plan.scratch_bytes(count, C), dtype=torch.uint8, device=dev)
        stage_in = torch.zeros(count * alpha * n, dtype=dt, device=dev)
        stage_out = torch.zeros(count * M * n, dtype=dt, device=dev)
        cfg_f = g.ntt_rns_configuration(n_power=logn, reduction_poly=g.X_N_plus)
        cfg_i = g.ntt_rns_configuration(n_power=logn, ntt_type=g.INVERSE, reduction_poly=g.X_N_plus, mod_inverse=d_ninv)

        def composed_mod_up(c, a):
            for d, S in enumerate(parts):
                rest = [m for m in range(M) if m not in S]
                for r in range(count):
                    for k, i in enumerate(S):
                        stage_in[(r * len(S) + k) * n:][:n].copy_(c[(r * L + i) * n:][:n])
                ups[d].convert(stage_in, stage_out, logn, count, g.CENTRED)
                for r in range(count):
                    stack = a[(d * count + r) * M * n:]
                    for k, i in enumerate(S):
                        stack[i * n:][:n].copy_(stage_in[(r * len(S) + k) * n:][:n])
                    for k, m in enumerate(rest):
                        stack[m * n:][:n].copy_(stage_out[(r * len(rest) + k) * n:][:n])

        def composed_mod_down(acc, out, stacks):
            for s in range(stacks):
                down.convert_and_divide(acc[(s * M + L) * n:], acc[s * M * n:], out[s * L * n:], logn, 1, g.CENTRED)

        def composed_apply(i):
            s = sets[i % nsets]
            composed_mod_up(s["c"], s["a"])
            g.GPU_NTT_Inplace(s["a"], d_fwd, d_mods, cfg_f, D * count * M, M)
            inner.multiply_accumulate(s["a"], s["key"], s["acc"], logn, D, C, count)
            g.GPU_INTT_Inplace(s["acc"], d_inv, d_mods, cfg_i, C * count * M, M)
            composed_mod_down(s["acc"], s["out"], C * count)

        col = count * n * wsz  # bytes of one limb of every input
        bytes_of = {"mod_up": (L + D * M) * col, "mod_down": C * (M + L) * col}
        # apply: mod_up, two in-place transforms (read + write each), the inner product, mod_down
        bytes_of["apply"] = bytes_of["mod_up"] + 2 * D * M * col + (D * M + C * M) * col + D * C * M * n * wsz + \
            2 * C * M * col + bytes_of["mod_down"]
        calls = {
            "mod_up": (lambda i: plan.mod_up(sets[i % nsets]["c"], sets[i % nsets]["a"], count),
                       lambda i: composed_mod_up(sets[i % nsets]["c"], sets[i % nsets]["a"])),
            "mod_down": (lambda i: plan.mod_down(sets[i % nsets]["acc"], sets[i % nsets]["out"], C * count),
                         lambda i: composed_mod_down(sets[i % nsets]["acc"], sets[i % nsets]["out"], C * count)),
            "apply": (lambda i: plan.apply(sets[i % nsets]["c"], sets[i % nsets]["key"], sets[i % nsets]["out"], count,
                                           C, False, False, scratch), composed_apply),
        }
        for op, (mine, theirs) in calls.items():
            half = bytes_of[op] // (2 * wsz)
            ncopy = max(2, -(-ROTATE_BYTES // bytes_of[op]) + 1)
            copies = [(torch.randint(0, 1 << 20, (half,), dtype=dt, device=dev), torch.empty(half, dtype=dt, device=dev))
                      for _ in range(ncopy)]
            res = {"case": name, "op": op, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "C": C,
                   "count": count, "algorithmic_bytes": bytes_of[op], "buffer_sets": nsets}
            res["calls_per_event_pair"] = args.calls
            res["copy_ms"] = median_ms(lambda i: copies[i % ncopy][1].copy_(copies[i % ncopy][0]), args.iters,
                                       calls=args.calls)
            del copies
            res["plan_ms"] = median_ms(mine, args.iters, calls=args.calls)
            res["composition_ms"] = median_ms(theirs, max(5, args.iters // 5), warmup=2)
            res["plan_over_copy"] = round(res["plan_ms"] / res["copy_ms"], 3)
            res["composition_over_plan"] = round(res["composition_ms"] / res["plan_ms"], 2)
            print(json.dumps(res), flush=True)
            lines.append(res)
        del sets, plan, inner, ups, down, scratch
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
