#!/usr/bin/env python3
"""BfvMultiplyPlan (include/gpuntt/rns/bfv_multiply.cuh), timed with bench_relin.py's method against what a
caller composes from the calls that existed before it.
  side (a)  multiply (NTT form in and out) against the composition: per operand the q-base INTT, BaseConvPlan.convert
            {q} -> {b} and the two strided copies that build the full-base stack; the full-base NTT; per input the three
            tensor terms through InnerProductPlan.multiply_accumulate (gathers for d1); the full-base INTT; side (b)'s
            composition; the q-base NTT
  side (b)  scale_round on 3 * count stacks against steps 1 to 3 of its definition: the multiplication by t as a full-base
            multiply_accumulate against a constant operand, two strided copies, convert_and_divide {q} -> {b}, convert
            {b} -> {q}
The transforms of the compositions are prepared NTTPlans, the conversions prepared BaseConvPlans, the gathers copy_ calls
into buffers that exist.  Before anything is timed, word equality of both sides with their compositions is checked.  Every
case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set.  Per case: warm-up,
then the median of --iters HIP event pairs, each around --calls back-to-back calls (the figure is per call), taken
--repeats times alternating the sides, so the spread of the baselines' own medians is recorded next to the ratios.  One
JSON line per case.
    python tools/bench_bfv.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/bfv_bench.jsonl]"""
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
from bench_relin import ROTATE_BYTES, median_ms  # noqa: E402
from bfv_utils import aux_count  # noqa: E402
from gpu_utils import find_ntt_factors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="calls per HIP event pair")
    ap.add_argument("--repeats", type=int, default=3, help="medians per side, alternating")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bfv.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, t, count
        ("u64_count1", 64, 16, 6, 65537, 1),
        ("u64_count16", 64, 16, 6, 65537, 16),
        ("u32_count16", 32, 14, 6, 65537, 16),
    ]
    lines = []
    for name, bits, logn, L, t, count in shapes:
        if args.only and name != args.only:
            continue
        n, wsz = 1 << logn, bits // 8
        dt = torch.int64 if bits == 64 else torch.int32
        npdt = g.np_dtype(bits)
        factors = [find_ntt_factors(59 if bits == 64 else 29, logn, skip=i, clear_of_top=True) for i in range(2 * L + 4)]
        K = aux_count([f[0] for f in factors], L, t, n)
        M = L + K
        prms = [g.NTTParameters(logn, g.X_N_plus, bits, f) for f in factors[:M]]
        fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
        for i, prm in enumerate(prms):
            fwd[i * n:i * n + prm.root_of_unity_size] = prm.forward_table_device_order
            inv[i * n:i * n + prm.root_of_unity_size] = prm.inverse_table_device_order
        qs = [p.modulus.value for p in prms]
        mods = [p.modulus for p in prms]
        ninv = [p.n_inv for p in prms]
        d_fwd, d_inv = g.to_device(fwd), g.to_device(inv)
        plan = g.BfvMultiplyPlan(qs[:L], qs[L:], t, logn, d_fwd, d_inv, ninv, g.X_N_plus, batch_hint=4 * count * M,
                                 bits=bits)
        intt_q = g.NTTPlan(d_inv, mods[:L], logn, g.X_N_plus, g.INVERSE, ninv[:L], batch_hint=2 * count * L)
        ntt_q = g.NTTPlan(d_fwd, mods[:L], logn, g.X_N_plus, g.FORWARD, ninv[:L], batch_hint=3 * count * L)
        ntt_full = g.NTTPlan(d_fwd, mods, logn, g.X_N_plus, g.FORWARD, ninv, batch_hint=4 * count * M)
        intt_full = g.NTTPlan(d_inv, mods, logn, g.X_N_plus, g.INVERSE, ninv, batch_hint=3 * count * M)
        up, down = g.BaseConvPlan(qs[:L], qs[L:], bits=bits), g.BaseConvPlan(qs[L:], qs[:L], bits=bits)
        inner = g.InnerProductPlan(qs, bits=bits)
        tconst = g.to_device(np.repeat(np.array([t % q for q in qs], dtype=npdt), n))  # T[M][N]
        stacks = 3 * count
        words = dict(x=2 * count * L * n, y=2 * count * L * n, out=stacks * L * n, coeff=2 * count * L * n,
                     conv=2 * count * K * n, e=4 * count * M * n, d=stacks * M * n, s=stacks * M * n, sq=stacks * L * n,
                     sb=stacks * K * n, r=stacks * K * n, ga=2 * M * n, gk=2 * M * n)
        sbytes = plan.scratch_bytes(count)
        per_set = sum(words.values()) * wsz + sbytes
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["scratch"] = torch.zeros(sbytes, dtype=torch.uint8, device=dev)

        def scale_round_composition(s, full, out):  # steps 1 to 3 of the definition
            inner.multiply_accumulate(full, tconst, s["s"], logn, 1, 1, stacks)
            v = s["s"].view(stacks, M, n)
            s["sq"].view(stacks, L, n).copy_(v[:, :L, :])
            s["sb"].view(stacks, K, n).copy_(v[:, L:, :])
            up.convert_and_divide(s["sq"], s["sb"], s["r"], logn, stacks, g.CENTRED)
            down.convert(s["r"], out, logn, stacks, g.CENTRED)

        def fused(i, out=None):
            s = sets[i % nsets]
            plan.multiply(s["x"], s["y"], s["out"] if out is None else out, count, True, True, s["scratch"])

        def composition(i, out=None):
            s = sets[i % nsets]
            out = s["out"] if out is None else out
            e = s["e"].view(2, 2 * count, M, n)
            for k, op in enumerate((s["x"], s["y"])):
                intt_q.execute(op, s["coeff"], 2 * count * L)
                up.convert(s["coeff"], s["conv"], logn, 2 * count, g.CENTRED)
                e[k, :, :L, :].copy_(s["coeff"].view(2 * count, L, n))
                e[k, :, L:, :].copy_(s["conv"].view(2 * count, K, n))
            ntt_full.execute(s["e"], s["e"], 4 * count * M)
            xe, ye = s["e"].view(2, 2, count, M, n)
            d, ga, gk = s["d"].view(3, count, M, n), s["ga"].view(2, M, n), s["gk"].view(2, M, n)
            for r in range(count):
                inner.multiply_accumulate(xe[0, r].reshape(-1), ye[0, r].reshape(-1), d[0, r].view(-1), logn, 1, 1, 1)
                ga[0].copy_(xe[0, r]), ga[1].copy_(xe[1, r]), gk[0].copy_(ye[1, r]), gk[1].copy_(ye[0, r])
                inner.multiply_accumulate(s["ga"], s["gk"], d[1, r].view(-1), logn, 2, 1, 1)
                inner.multiply_accumulate(xe[1, r].reshape(-1), ye[1, r].reshape(-1), d[2, r].view(-1), logn, 1, 1, 1)
            intt_full.execute(s["d"], s["d"], stacks * M)
            scale_round_composition(s, s["d"], out)
            ntt_q.execute(out, out, stacks * L)

        def scale_round(i, out=None):
            s = sets[i % nsets]
            plan.scale_round(s["d"], s["out"] if out is None else out, stacks)

        def scale_round_steps(i, out=None):
            s = sets[i % nsets]
            scale_round_composition(s, s["d"], s["out"] if out is None else out)

        a, b = (torch.empty(stacks * L * n, dtype=dt, device=dev) for _ in range(2))
        scale_round(0, a), scale_round_steps(0, b)  # before `composition` rewrites d of set 0
        torch.cuda.synchronize()
        same_scale_round = bool(torch.equal(a, b))
        fused(0, a), composition(0, b)
        torch.cuda.synchronize()
        same_multiply = bool(torch.equal(a, b))
        del a, b
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "plain_modulus": t, "count": count,
               "input_ntt": True, "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls,
               "multiply_matches_its_composition": same_multiply,
               "scale_round_matches_its_composition": same_scale_round,
               # words per column that cross the memory interface
               "scale_round_words_per_column": {"fused": M + L, "steps": 3 * M + 2 * K + L}}
        tm = {k: [] for k in ("composition", "multiply", "scale_round_steps", "scale_round")}
        for _ in range(args.repeats):  # alternating, so every side sees the same neighbours on the machine
            tm["composition"].append(median_ms(composition, args.iters, calls=args.calls))
            tm["multiply"].append(median_ms(fused, args.iters, calls=args.calls))
            tm["scale_round_steps"].append(median_ms(scale_round_steps, args.iters, calls=args.calls))
            tm["scale_round"].append(median_ms(scale_round, args.iters, calls=args.calls))
        for k, v in tm.items():
            res[k + "_ms"] = [round(x, 5) for x in v]
        med = {k: float(np.median(v)) for k, v in tm.items()}
        res["multiply_over_composition"] = round(med["multiply"] / med["composition"], 3)
        res["composition_spread"] = round((max(tm["composition"]) - min(tm["composition"])) / med["composition"], 3)
        res["scale_round_over_steps"] = round(med["scale_round"] / med["scale_round_steps"], 3)
        res["scale_round_steps_spread"] = round(
            (max(tm["scale_round_steps"]) - min(tm["scale_round_steps"])) / med["scale_round_steps"], 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan, up, down, inner, intt_q, ntt_q, ntt_full, intt_full
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
