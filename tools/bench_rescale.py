#!/usr/bin/env python3
"""The rescaling calls of KeySwitchPlan (include/gpuntt/rns/key_switch.cuh), timed with bench_relin.py's
method against what a caller composes from the calls that existed before them.
  side (a)  multiply_relinearize_rescale against
              composition 1: multiply_relinearize(output_ntt=True), INTT over L, gathers, convert_and_divide, NTT over L'
              composition 2: multiply_relinearize(output_ntt=False), gathers, convert_and_divide, NTT over L'
            the ratio is taken against the faster of the two
  side (b)  rescale(ntt_form=True) on 2 * count stacks against INTT over L, gathers, convert_and_divide, NTT over L'
The transforms of the compositions are prepared NTTPlans, the conversion a prepared BaseConvPlan, the gathers two strided
copy_ calls into buffers that exist.  Before anything is timed, word equality is checked wherever the definitions promise
it: composition 1 against composition 2, side (b) against its composition; the fused product rounds once where the
compositions round twice, so it is checked to lie within 1 of them per coefficient instead (key_switch.cuh).  Every case
rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set.  Per case: warm-up, then
the median of --iters HIP event pairs, each around --calls back-to-back calls (the figure is per call), taken --repeats
times alternating the sides, so the spread of the baselines' own medians is recorded next to the ratios.  One JSON line
per case.
    python tools/bench_rescale.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/rescale_bench.jsonl]"""
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
        sys.exit("bench_rescale.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, L, K, alpha, R, count
        ("u64_count1", 64, 16, 6, 2, 2, 1, 1),
        ("u64_count16", 64, 16, 6, 2, 2, 1, 16),
        ("u32_count16", 32, 14, 6, 2, 2, 2, 16),
    ]
    lines = []
    for name, bits, logn, L, K, alpha, R, count in shapes:
        if args.only and name != args.only:
            continue
        M, n, wsz, Lk, stacks = L + K, 1 << logn, bits // 8, L - R, 2 * count
        D = -(-L // alpha)
        dt = torch.int64 if bits == 64 else torch.int32
        npdt = g.np_dtype(bits)
        prms = []
        fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
        for i in range(M):
            f = find_ntt_factors(59 if bits == 64 else 29, logn, skip=i, clear_of_top=True)
            prm = g.NTTParameters(logn, g.X_N_plus, bits, f)
            prms.append(prm)
            fwd[i * n:i * n + prm.root_of_unity_size] = prm.forward_table_device_order
            inv[i * n:i * n + prm.root_of_unity_size] = prm.inverse_table_device_order
        qs = [p.modulus.value for p in prms]
        mods = [p.modulus for p in prms]
        ninv = [p.n_inv for p in prms]
        d_fwd, d_inv = g.to_device(fwd), g.to_device(inv)
        plain = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, d_fwd, d_inv, ninv, g.X_N_plus,
                                batch_hint=D * count * M, bits=bits)
        plan = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, d_fwd, d_inv, ninv, g.X_N_plus,
                               batch_hint=D * count * M, bits=bits, rescale_limbs=R)
        intt_q = g.NTTPlan(d_inv, mods[:L], logn, g.X_N_plus, g.INVERSE, ninv[:L], batch_hint=stacks * L)
        ntt_keep = g.NTTPlan(d_fwd, mods[:Lk], logn, g.X_N_plus, g.FORWARD, ninv[:Lk], batch_hint=stacks * Lk)
        conv = g.BaseConvPlan(qs[Lk:L], qs[:Lk], bits=bits)
        key = torch.randint(0, min(qs), (D * 2 * M * n,), dtype=dt, device=dev)
        ct, small = stacks * L * n, stacks * Lk * n
        words = dict(x=ct, y=ct, full=ct, out=small, dropped=stacks * R * n, kept=small)
        sbytes, rbytes = plan.scratch_bytes(count, 2), plan.rescale_scratch_bytes(stacks)
        per_set = sum(words.values()) * wsz + sbytes + rbytes
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(qs), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["scratch"] = torch.zeros(sbytes, dtype=torch.uint8, device=dev)
            s["rscratch"] = torch.zeros(rbytes, dtype=torch.uint8, device=dev)

        def divide(s, src, out):  # gathers, convert_and_divide, NTT over the kept limbs
            v = src.view(stacks, L, n)
            s["dropped"].view(stacks, R, n).copy_(v[:, Lk:, :])
            s["kept"].view(stacks, Lk, n).copy_(v[:, :Lk, :])
            conv.convert_and_divide(s["dropped"], s["kept"], out, logn, stacks, g.CENTRED)
            ntt_keep.execute(out, out, stacks * Lk)

        def fused(i, out=None):
            s = sets[i % nsets]
            plan.multiply_relinearize_rescale(s["x"], s["y"], key, s["out"] if out is None else out, count, True,
                                              s["scratch"])

        def composition1(i, out=None):
            s = sets[i % nsets]
            plain.multiply_relinearize(s["x"], s["y"], key, s["full"], count, True, s["scratch"])
            intt_q.execute(s["full"], s["full"], stacks * L)
            divide(s, s["full"], s["out"] if out is None else out)

        def composition2(i, out=None):
            s = sets[i % nsets]
            plain.multiply_relinearize(s["x"], s["y"], key, s["full"], count, False, s["scratch"])
            divide(s, s["full"], s["out"] if out is None else out)

        def rescale(i, out=None):
            s = sets[i % nsets]
            plan.rescale(s["x"], s["out"] if out is None else out, stacks, True, s["rscratch"])

        def rescale_composition(i, out=None):
            s = sets[i % nsets]
            intt_q.execute(s["x"], s["full"], stacks * L)
            divide(s, s["full"], s["out"] if out is None else out)

        a, b, c = (torch.empty(small, dtype=dt, device=dev) for _ in range(3))
        fused(0, a), composition1(0, b), composition2(0, c)
        torch.cuda.synchronize()
        same12 = bool(torch.equal(b, c))
        # both results are coefficient-wise comparable only in coefficient form: inverse-transform the kept limbs
        intt_keep = g.NTTPlan(d_inv, mods[:Lk], logn, g.X_N_plus, g.INVERSE, ninv[:Lk], batch_hint=stacks * Lk)
        intt_keep.execute(a, a, stacks * Lk), intt_keep.execute(b, b, stacks * Lk)
        torch.cuda.synchronize()
        qt = g.to_device(np.array(qs[:Lk], dtype=npdt)).view(1, Lk, 1)
        diff = (a.view(stacks, Lk, n) - b.view(stacks, Lk, n)) % qt  # the same integer in every kept limb: -1, 0 or 1
        small_diff = (diff == 0) | (diff == 1) | (diff == qt - 1)
        sign = torch.where(diff == qt - 1, -1, diff)
        within_one = bool(small_diff.all()) and bool((sign == sign[:, :1, :]).all())
        rescale(0, a), rescale_composition(0, b)
        torch.cuda.synchronize()
        same_rescale = bool(torch.equal(a, b))
        del a, b, c, diff, small_diff, sign
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha,
               "rescale_limbs": R, "count": count, "output_ntt": True, "buffer_sets": nsets,
               "calls_per_event_pair": args.calls, "compositions_agree": same12,
               "fused_within_one_of_the_compositions": within_one, "rescale_matches_its_composition": same_rescale,
               # per stack: transforms after the inner product, and passes over dense arrays
               "transforms_per_stack": {"fused": M + Lk, "composition1": M + L + L + Lk, "composition2": M + Lk,
                                        "rescale": R + Lk, "rescale_composition": L + Lk}}
        t = {k: [] for k in ("fused", "composition1", "composition2", "rescale", "rescale_composition")}
        for _ in range(args.repeats):  # alternating, so every side sees the same neighbours on the machine
            t["composition1"].append(median_ms(composition1, args.iters, calls=args.calls))
            t["composition2"].append(median_ms(composition2, args.iters, calls=args.calls))
            t["fused"].append(median_ms(fused, args.iters, calls=args.calls))
            t["rescale_composition"].append(median_ms(rescale_composition, args.iters, calls=args.calls))
            t["rescale"].append(median_ms(rescale, args.iters, calls=args.calls))
        for k, v in t.items():
            res[k + "_ms"] = [round(x, 5) for x in v]
        med = {k: float(np.median(v)) for k, v in t.items()}
        faster = "composition1" if med["composition1"] < med["composition2"] else "composition2"
        res["faster_composition"] = faster
        res["fused_over_faster_composition"] = round(med["fused"] / med[faster], 3)
        res["faster_composition_spread"] = round((max(t[faster]) - min(t[faster])) / med[faster], 3)
        res["rescale_over_composition"] = round(med["rescale"] / med["rescale_composition"], 3)
        res["rescale_composition_spread"] = round(
            (max(t["rescale_composition"]) - min(t["rescale_composition"])) / med["rescale_composition"], 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del sets, plan, plain, key, conv, intt_q, ntt_keep, intt_keep
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
