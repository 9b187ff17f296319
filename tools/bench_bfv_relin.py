#!/usr/bin/env python3
"""BfvMultiplyPlan.multiply_relinearize and KeySwitchPlan.relinearize, timed with bench_bfv.py's method
against what a caller composes from the public calls that existed before them.
  side (a)  multiply_relinearize against: multiply(output_ntt = false) into a T[3][count][L][N] temporary; apply on its top
            component (input_ntt = false, output_ntt); with the result in NTT form the q-base NTT of the two low
            components; the two modular additions
  side (b)  relinearize on a three-component ciphertext against apply plus the two additions (the operands already in
            the form of the result)
The additions are bench_relin.py's: one torch addition and one torch.where per call, the caller's own add pass -- the
library had none.  Since a caller's add kernel could be cheaper than that, every case also records the composition WITHOUT
the additions (a free add pass): the ratio against it is the conservative one.  Both forms are measured: operands and
result in NTT form, and in coefficient form.  Before anything is timed, word equality of both sides is checked.  Every case
rotates over enough distinct buffer sets that more than 512 MiB pass between two uses of a set.  Per case: warm-up, then
the median of --iters HIP event pairs, each around --calls back-to-back calls (the figure is per call), taken --repeats
times alternating the sides, so the spread of the baselines' own medians is recorded next to the ratios.  One JSON line per
case.
    python tools/bench_bfv_relin.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/bfv_relin_bench.jsonl]"""
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
        sys.exit("bench_bfv_relin.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    K_p, alpha = 2, 2
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
                   for i in range(2 * L + 4 + K_p)]
        K_b = aux_count([f[0] for f in factors[:2 * L + 4]], L, t, n)
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
        bfv = g.BfvMultiplyPlan(bq[:L], bq[L:], t, logn, b_fwd, b_inv, b_ninv, g.X_N_plus, batch_hint=4 * count * M_b,
                                bits=bits)
        ks = g.KeySwitchPlan(pq[:L], pq[L:], alpha, logn, p_fwd, p_inv, p_ninv, g.X_N_plus,
                             batch_hint=ks_batch(L, alpha, count, M_p), bits=bits)
        ntt_q = g.NTTPlan(p_fwd, pmods[:L], logn, g.X_N_plus, g.FORWARD, p_ninv[:L], batch_hint=2 * count * L)
        qt = g.to_device(np.array(bq[:L], dtype=npdt)).view(1, 1, L, 1)
        low, top = 2 * count * L * n, count * L * n
        key = torch.randint(0, min(pq), ((ks.digits * 2 * M_p) << logn,), dtype=dt, device=dev)
        words = dict(x=low, y=low, out=low, three=low + top, k=low, ct=low + top)
        sb, kb = bfv.scratch_bytes(count), ks.scratch_bytes(count, 2)
        per_set = sum(words.values()) * wsz + sb + kb
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = [{k: torch.randint(0, min(bq[:L]), (w,), dtype=dt, device=dev) for k, w in words.items()}
                for _ in range(nsets)]
        for s in sets:
            s["scratch"] = torch.zeros(sb, dtype=torch.uint8, device=dev)
            s["ks_scratch"] = torch.zeros(kb, dtype=torch.uint8, device=dev)

        def add(k, lowc, out):  # the caller's two modular additions
            v = k.view(2, count, L, n) + lowc.view(2, count, L, n)
            torch.where(v >= qt, v - qt, v, out=out.view(2, count, L, n))

        def sides(ntt, additions):
            def fused(i, out=None):
                s = sets[i % nsets]
                bfv.multiply_relinearize(s["x"], s["y"], ks, key, s["out"] if out is None else out, count, ntt, ntt,
                                         s["scratch"], s["ks_scratch"])

            def composition(i, out=None):
                s = sets[i % nsets]
                bfv.multiply(s["x"], s["y"], s["three"], count, ntt, False, s["scratch"])
                ks.apply(s["three"][low:], key, s["k"], count, 2, False, ntt, s["ks_scratch"])
                if ntt:
                    ntt_q.execute(s["three"][:low], s["three"][:low], 2 * count * L)
                if additions:
                    add(s["k"], s["three"][:low], s["out"] if out is None else out)

            def relinearize(i, out=None):
                s = sets[i % nsets]
                ks.relinearize(s["ct"][:low], s["ct"][low:], key, s["out"] if out is None else out, count, ntt, ntt,
                               s["ks_scratch"])

            def apply_and_add(i, out=None):
                s = sets[i % nsets]
                ks.apply(s["ct"][low:], key, s["k"], count, 2, ntt, ntt, s["ks_scratch"])
                if additions:
                    add(s["k"], s["ct"][:low], s["out"] if out is None else out)
            return fused, composition, relinearize, apply_and_add

        for ntt in (True, False):
            fused, composition, relinearize, apply_and_add = sides(ntt, True)
            _, composition_bare, _, apply_bare = sides(ntt, False)
            a, b = (torch.empty(low, dtype=dt, device=dev) for _ in range(2))
            fused(0, a), composition(0, b)
            torch.cuda.synchronize()
            same_bfv = bool(torch.equal(a, b))
            relinearize(0, a), apply_and_add(0, b)
            torch.cuda.synchronize()
            same_relin = bool(torch.equal(a, b))
            del a, b
            res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K_b": K_b, "K_p": K_p, "alpha": alpha,
                   "plain_modulus": t, "count": count, "ntt_form": ntt, "buffer_sets": nsets,
                   "calls_per_event_pair": args.calls, "multiply_relinearize_matches_its_composition": same_bfv,
                   "relinearize_matches_its_composition": same_relin}
            fns = {"composition": composition, "composition_without_additions": composition_bare,
                   "multiply_relinearize": fused, "apply_and_add": apply_and_add, "apply": apply_bare,
                   "relinearize": relinearize}
            tm = {k: [] for k in fns}
            for _ in range(args.repeats):  # alternating, so every side sees the same neighbours on the machine
                for k, fn in fns.items():
                    tm[k].append(median_ms(fn, args.iters, calls=args.calls))
            for k, v in tm.items():
                res[k + "_ms"] = [round(x, 5) for x in v]
            med = {k: float(np.median(v)) for k, v in tm.items()}
            res["multiply_relinearize_over_composition"] = round(med["multiply_relinearize"] / med["composition"], 3)
            res["multiply_relinearize_over_composition_without_additions"] = round(
                med["multiply_relinearize"] / med["composition_without_additions"], 3)
            res["composition_spread"] = round((max(tm["composition"]) - min(tm["composition"])) / med["composition"], 3)
            res["relinearize_over_apply_and_add"] = round(med["relinearize"] / med["apply_and_add"], 3)
            res["relinearize_over_apply"] = round(med["relinearize"] / med["apply"], 3)
            res["apply_and_add_spread"] = round(
                (max(tm["apply_and_add"]) - min(tm["apply_and_add"])) / med["apply_and_add"], 3)
            print(json.dumps(res), flush=True)
            lines.append(res)
        del sets, bfv, ks, ntt_q
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def ks_batch(L, alpha, count, M):
    """the widest transform of a key switch: D * count * M polynomials"""
    return -(-L // alpha) * count * M


if __name__ == "__main__":
    main()
