#!/usr/bin/env python3
"""BfvMultiplyPlan.multiply_relinearize_sum, timed with bench_bfv_relin.py's method against what a caller
had before it: `terms` calls of multiply_relinearize and terms - 1 modular additions.
  sum                        multiply_relinearize_sum over `terms` pairs of distinct ciphertexts, one call
  separate                   `terms` calls of multiply_relinearize on the same plan, plus the caller's terms - 1 additions
                             (bench_relin.py's: one torch addition and one torch.where each -- the library has no add call)
  separate_without_additions the same with the additions counted as free: the ratio against it is the conservative one
At terms = 1 `separate` is multiply_relinearize itself, so the ratio is the cost of the term loop.  Both forms are measured:
operands and result in NTT form, and in coefficient form.  The auxiliary base is the smallest that holds the largest
`terms` timed, and all sides use that one plan.
Checked before anything is timed.  (1) terms = 1: the words of multiply_relinearize.  (2) The two sides are not word for word
equal for terms > 1 -- one rounding against `terms` -- and the relinearized words are not close either (bfv_multiply.cuh),
so the rounding bound is checked where the header states it: multiply_sum against the sum of `terms` multiply results, the
centred CRT difference at --check-columns sampled columns of every component and input, against
(terms + 1) / 2 + terms + 1.
Every case rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set.  Per case:
warm-up, then the median of --iters HIP event pairs, each around --calls back-to-back calls (the figure is per call), taken
--repeats times alternating the sides.  One JSON line per case.
    python tools/bench_bfv_sum.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/bfv_sum_bench.jsonl]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import _load_pkg  # noqa: E402
from bench_bfv_relin import ks_batch  # noqa: E402
from bench_relin import ROTATE_BYTES, median_ms  # noqa: E402
from bfv_utils import aux_count  # noqa: E402
from gpu_utils import find_ntt_factors  # noqa: E402

TERMS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="calls per HIP event pair")
    ap.add_argument("--repeats", type=int, default=3, help="medians per side, alternating")
    ap.add_argument("--check-columns", type=int, default=64, help="columns of the rounding check")
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--note", default=None, help="recorded in every line (the variant of an A/B)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bfv_sum.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    K_p, alpha, most = 2, 2, max(TERMS)
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
        factors = [find_ntt_factors(59 if bits == 64 else 29, logn, skip=i, clear_of_top=True)
                   for i in range(2 * L + 6 + K_p)]
        K_b = aux_count([f[0] for f in factors[:2 * L + 6]], L, t * most, n)
        prms = [g.NTTParameters(logn, g.X_N_plus, bits, f) for f in factors]

        def stack(idx):  # the moduli idx as one full base: values, Modulus objects, tables on the device, n^-1
            fwd, inv = np.zeros(len(idx) * n, dtype=npdt), np.zeros(len(idx) * n, dtype=npdt)
            for k, i in enumerate(idx):
                fwd[k * n:k * n + prms[i].root_of_unity_size] = prms[i].forward_table_device_order
                inv[k * n:k * n + prms[i].root_of_unity_size] = prms[i].inverse_table_device_order
            return ([prms[i].modulus.value for i in idx], [prms[i].modulus for i in idx], g.to_device(fwd),
                    g.to_device(inv), [prms[i].n_inv for i in idx])
        q_idx = list(range(L))
        bq, bmods, b_fwd, b_inv, b_ninv = stack(q_idx + list(range(L, L + K_b)))
        pq, pmods, p_fwd, p_inv, p_ninv = stack(q_idx + list(range(L + K_b, L + K_b + K_p)))
        M_b, M_p = L + K_b, L + K_p
        # the batch hint of bench_bfv_relin.py: the one that suits the separate calls, not the wider batch of the sum
        bfv = g.BfvMultiplyPlan(bq[:L], bq[L:], t, logn, b_fwd, b_inv, b_ninv, g.X_N_plus, batch_hint=4 * count * M_b,
                                bits=bits)
        assert bfv.max_terms >= most
        ks = g.KeySwitchPlan(pq[:L], pq[L:], alpha, logn, p_fwd, p_inv, p_ninv, g.X_N_plus,
                             batch_hint=ks_batch(L, alpha, count, M_p), bits=bits)
        qs = bq[:L]
        Q = math.prod(qs)
        qt = g.to_device(np.array(qs, dtype=npdt)).view(1, 1, L, 1)
        low = 2 * count * L * n
        key = torch.randint(0, min(pq), ((ks.digits * 2 * M_p) << logn,), dtype=dt, device=dev)
        sb, kb = bfv.sum_scratch_bytes(count, 2 * most), ks.scratch_bytes(count, 2)
        per_set = (2 * most + 2) * low * wsz + sb + kb
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = []
        for _ in range(nsets):
            s = {"x": [torch.randint(0, min(qs), (low,), dtype=dt, device=dev) for _ in range(most)],
                 "y": [torch.randint(0, min(qs), (low,), dtype=dt, device=dev) for _ in range(most)],
                 "out": torch.empty(low, dtype=dt, device=dev), "part": torch.empty(low, dtype=dt, device=dev),
                 "scratch": torch.zeros(sb, dtype=torch.uint8, device=dev),
                 "ks_scratch": torch.zeros(kb, dtype=torch.uint8, device=dev)}
            sets.append(s)

        def add(acc, part):  # the caller's modular addition, in place on acc
            v = acc.view(2, count, L, n) + part.view(2, count, L, n)
            torch.where(v >= qt, v - qt, v, out=acc.view(2, count, L, n))

        def sides(terms, ntt, additions):
            def fused(i, out=None):
                s = sets[i % nsets]
                bfv.multiply_relinearize_sum(s["x"][:terms], s["y"][:terms], ks, key, s["out"] if out is None else out,
                                             count, ntt, ntt, s["scratch"], s["ks_scratch"])

            def separate(i, out=None):
                s = sets[i % nsets]
                acc = s["out"] if out is None else out
                for k in range(terms):
                    bfv.multiply_relinearize(s["x"][k], s["y"][k], ks, key, acc if k == 0 else s["part"], count, ntt,
                                             ntt, s["scratch"], s["ks_scratch"])
                    if k and additions:
                        add(acc, s["part"])
            return fused, separate

        def crt_columns(tensor, comps, cols):
            """the centred-ready integers of the sampled columns: [comps * count][len(cols)] Python ints modulo Q"""
            h = g.to_host(tensor).reshape(comps * count, L, n)[:, :, cols].astype(object)
            out = np.zeros((comps * count, len(cols)), dtype=object)
            for i, q in enumerate(qs):
                out += h[:, i, :] * ((Q // q) * pow(Q // q, -1, q))
            return out % Q

        cols = np.unique(np.linspace(0, n - 1, args.check_columns).astype(np.int64))
        for ntt in (True, False):
            for terms in TERMS:
                fused, separate = sides(terms, ntt, True)
                _, separate_bare = sides(terms, ntt, False)
                res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K_b": K_b, "K_p": K_p, "alpha": alpha,
                       "plain_modulus": t, "count": count, "terms": terms, "ntt_form": ntt, "buffer_sets": nsets,
                       "calls_per_event_pair": args.calls}
                if args.note:
                    res["note"] = args.note
                # the checks: the words of multiply_relinearize at one term; the rounding bound on the three components
                s = sets[0]
                if terms == 1:
                    a, b = (torch.empty(low, dtype=dt, device=dev) for _ in range(2))
                    fused(0, a), separate(0, b)
                    torch.cuda.synchronize()
                    res["one_term_matches_multiply_relinearize"] = bool(torch.equal(a, b))
                    del a, b
                three, part = (torch.empty(3 * count * L * n, dtype=dt, device=dev) for _ in range(2))
                bfv.multiply_sum(s["x"][:terms], s["y"][:terms], three, count, ntt, False, s["scratch"])
                torch.cuda.synchronize()
                total = np.zeros((3 * count, len(cols)), dtype=object)
                for k in range(terms):
                    bfv.multiply(s["x"][k], s["y"][k], part, count, ntt, False, s["scratch"])
                    torch.cuda.synchronize()
                    total += crt_columns(part, 3, cols)
                diff = (crt_columns(three, 3, cols) - total) % Q
                worst = max(min(int(d), Q - int(d)) for d in diff.reshape(-1))
                bound = (terms + 1) / 2 + terms + 1
                res["rounding_difference_max"], res["rounding_bound"] = worst, bound
                res["within_rounding_bound"] = bool(worst <= bound)
                del three, part
                if not res["within_rounding_bound"] or res.get("one_term_matches_multiply_relinearize") is False:
                    print(json.dumps(res), flush=True)
                    sys.exit("a side is wrong: nothing is timed")
                fns = {"separate": separate, "separate_without_additions": separate_bare, "sum": fused}
                tm = {k: [] for k in fns}
                for _ in range(args.repeats):  # alternating, so every side sees the same neighbours on the machine
                    for k, fn in fns.items():
                        tm[k].append(median_ms(fn, args.iters, calls=args.calls))
                for k, v in tm.items():
                    res[k + "_ms"] = [round(x, 5) for x in v]
                med = {k: float(np.median(v)) for k, v in tm.items()}
                res["sum_over_separate"] = round(med["sum"] / med["separate"], 3)
                res["sum_over_separate_without_additions"] = round(med["sum"] / med["separate_without_additions"], 3)
                res["separate_spread"] = round((max(tm["separate"]) - min(tm["separate"])) / med["separate"], 3)
                print(json.dumps(res), flush=True)
                lines.append(res)
        del sets, bfv, ks
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
