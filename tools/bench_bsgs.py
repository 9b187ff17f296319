#!/usr/bin/env python3
"""KeySwitchPlan.linear_transform_bsgs (include/gpuntt/rns/key_switch.cuh), timed at the shapes of DESIGN.md 3.18 against
BOTH things a caller could do before it:
  (A) one rotate_hoisted_sum with G = n1 * n2 keys -- not a baby-step/giant-step product at all, possible while G <= 64;
  (B) single-hoisted BSGS from the public calls: n2 x rotate_hoisted_sum over the n1 baby steps, then per keyed giant step
      decompose + rotate_hoisted_sum(G = 1).  The caller's own modular additions of the n2 results are LEFT OUT (the
      library has no call for them), so B is a lower bound of that path.
The three do not produce the same words (they round at different places), so before anything is timed the tool checks
the new call against its own definition, tests/bsgs_utils.composition_bsgs, once per case -- at count = min(count, 2):
the definition's P c products are Python integers.  Every case rotates over enough distinct buffer sets that more than
512 MiB pass between two uses of a set: every timed call reads from HBM.  Per case: warm-up, then the median of --iters
HIP event pairs, each around --calls back-to-back calls (the figure is per call), taken --repeats times alternating the
sides.  One JSON line per case.
    python tools/bench_bsgs.py [--iters 20] [--calls 5] [--repeats 3] [--out profiles/bsgs_bench.jsonl]"""
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
from bsgs_utils import composition_bsgs  # noqa: E402
from gpu_utils import find_ntt_factors  # noqa: E402

ROTATE_BYTES = 512 << 20
SCRATCH_CAP = 4 << 30


def median_ms(fn, iters, warmup=2, calls=1):
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
        sys.exit("bench_bsgs.py needs a GPU: nothing is measured without one")
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    L, K, alpha = 6, 2, 2
    shapes = [("u64_count1", 64, 16, 1), ("u32_count16", 32, 14, 16), ("u64_largest", 64, 16, None)]
    rings, sink = {}, None
    if args.out:  # one line per case as it finishes
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        sink = open(args.out, "w")
    for (name, bits, logn, count), (n1, n2) in ((s, d) for s in shapes for d in ((4, 4), (8, 8))):
        case = "%s_%dx%d" % (name, n1, n2)
        if args.only and case != args.only:
            continue
        M, n, wsz = L + K, 1 << logn, bits // 8
        D = -(-L // alpha)
        dt = torch.int64 if bits == 64 else torch.int32
        npdt = g.np_dtype(bits)
        if (bits, logn) not in rings:  # the primes and their tables, once per ring
            prms = [g.NTTParameters(logn, g.X_N_plus, bits,
                                    find_ntt_factors(59 if bits == 64 else 29, logn, skip=i, clear_of_top=True))
                    for i in range(M)]
            fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
            for i, prm in enumerate(prms):
                fwd[i * n:i * n + prm.root_of_unity_size] = prm.forward_table_device_order
                inv[i * n:i * n + prm.root_of_unity_size] = prm.inverse_table_device_order
            rings[(bits, logn)] = (prms, fwd, inv)
        prms, fwd, inv = rings[(bits, logn)]
        qs = [p.modulus.value for p in prms]
        ninv = [p.n_inv for p in prms]
        d_fwd, d_inv = g.to_device(fwd), g.to_device(inv)
        plan = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, d_fwd, d_inv, ninv, g.X_N_plus, batch_hint=2 * 16 * M,
                               bits=bits)
        if count is None:  # the largest count <= 16 whose scratch stays under 4 GiB
            count = max(c for c in range(1, 17) if plan.bsgs_scratch_bytes(c, n1, n2) < SCRATCH_CAP)
        G = n1 * n2

        def rnd(words):
            return torch.randint(0, min(qs), (words,), dtype=dt, device=dev)
        # keys and weights are shared by every buffer set (what a linear transform keeps resident)
        key_words, weight_words = D * 2 * M * n, M * n
        belts = [1] + [g.galois_element_for_rotation(s, logn) for s in range(1, n1)]
        gelts = [1] + [g.galois_element_for_rotation(s * n1, logn) for s in range(1, n2)]
        bkeys, gkeys = [rnd(key_words) for _ in range(n1)], [rnd(key_words) for _ in range(n2)]
        weights = [[rnd(weight_words) for _ in range(n1)] for _ in range(n2)]
        flat_w = [w for row in weights for w in row]
        with_a = G <= 64
        # (A) needs one key per diagonal: G = n1 * n2 of them
        a_keys = bkeys + gkeys + [rnd(key_words) for _ in range(G - n1 - n2)] if with_a else []
        a_elts = [g.galois_element_for_rotation(s, logn) for s in range(G)]
        words = dict(a=D * count * M * n, c0=count * L * n, c1=count * L * n, out=2 * count * L * n,
                     parts=n2 * 2 * count * L * n, a2=D * count * M * n)
        sbytes = dict(bsgs=plan.bsgs_scratch_bytes(count, n1, n2), sum=plan.hoisted_sum_scratch_bytes(count),
                      ks=plan.scratch_bytes(count, 2))
        per_set = sum(words.values()) * wsz + sum(sbytes.values())
        nsets = max(2, -(-ROTATE_BYTES // per_set) + 1)
        sets = []
        for _ in range(nsets):
            s = {k: rnd(w) for k, w in words.items()}
            s.update({k: torch.zeros(b, dtype=torch.uint8, device=dev) for k, b in sbytes.items()})
            sets.append(s)
        nb, ng = [None] + bkeys[1:], [None] + gkeys[1:]  # the b = 0 and g = 0 steps take no key

        def bsgs(i):
            s = sets[i % nsets]
            plan.linear_transform_bsgs(s["a"], s["c0"], s["c1"], nb, belts, ng, gelts, weights, s["out"], count, True,
                                       s["bsgs"])

        def side_a(i):
            s = sets[i % nsets]
            plan.rotate_hoisted_sum(s["a"], s["c0"], a_keys, a_elts, flat_w, s["out"], count, True, s["sum"])

        def side_b(i):
            s = sets[i % nsets]
            part = s["parts"].view(n2, -1)
            for gi in range(n2):
                plan.rotate_hoisted_sum(s["a"], s["c0"], bkeys, belts, weights[gi], part[gi], count, True, s["sum"])
            half = count * L * n
            for gi in range(1, n2):
                plan.decompose(part[gi][half:], s["a2"], count, True, s["ks"])
                plan.rotate_hoisted_sum(s["a2"], part[gi][:half], [gkeys[gi]], [gelts[gi]], None, s["out"], count, True,
                                        s["sum"])

        # the call against its definition, on the plan and the operands of the case, at a count the host part can afford
        cc = min(count, 2)
        st = dict(moduli=qs, poly=g.X_N_plus, mods=g.modulus_array_to_device([p.modulus for p in prms], bits),
                  fwd=d_fwd, inv=d_inv, d_ninv=g.to_device(np.array(ninv, dtype=npdt)))
        s0 = sets[0]
        ca, c0, c1 = rnd(D * cc * M * n), rnd(cc * L * n), rnd(cc * L * n)
        check = torch.empty(2 * cc * L * n, dtype=dt, device=dev)
        plan.linear_transform_bsgs(ca, c0, c1, nb, belts, ng, gelts, weights, check, cc, True, s0["bsgs"])
        torch.cuda.synchronize()
        same = bool(torch.equal(check, composition_bsgs(g, plan, st, ca, c0, c1, nb, belts, ng, gelts, weights, cc, True)))
        del check, ca, c0, c1
        key_unit = D * 2 * M * n  # words per switching key (key_mod_count = M)
        res = {"case": case, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "n1": n1, "n2": n2,
               "count": count, "output_ntt": True, "buffer_sets": nsets, "calls_per_event_pair": args.calls,
               "matches_its_definition": same, "definition_checked_at_count": cc,
               "scratch_bytes": sbytes["bsgs"],
               "key_words": {"bsgs": (n1 + n2 - 2) * key_unit, "single_hoisted": (n1 + n2) * key_unit,
                             "one_hoisted_sum": G * key_unit}}
        mine, ta, tb = [], [], []
        for _ in range(args.repeats):  # alternating, so all sides see the same neighbours on the machine
            if with_a:
                ta.append(median_ms(side_a, args.iters, calls=args.calls))
            tb.append(median_ms(side_b, args.iters, calls=args.calls))
            mine.append(median_ms(bsgs, args.iters, calls=args.calls))
        res["bsgs_ms"] = [round(v, 5) for v in mine]
        res["one_hoisted_sum_ms"] = [round(v, 5) for v in ta]
        res["single_hoisted_lower_bound_ms"] = [round(v, 5) for v in tb]
        res["bsgs_over_one_hoisted_sum"] = round(float(np.median(mine)) / float(np.median(ta)), 3) if ta else None
        res["bsgs_over_single_hoisted"] = round(float(np.median(mine)) / float(np.median(tb)), 3)
        res["single_hoisted_spread"] = round((max(tb) - min(tb)) / float(np.median(tb)), 3)
        print(json.dumps(res), flush=True)
        if sink:
            sink.write(json.dumps(res) + "\n")
            sink.flush()
        del sets, plan, bkeys, gkeys, weights, flat_w, a_keys, nb, ng
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
