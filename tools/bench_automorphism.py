#!/usr/bin/env python3
"""Galois automorphisms (include/gpuntt/ntt_merge/galois.cuh), timed: the NTT-domain permutation and the
coefficient-domain call at the benchmark's shapes, against a same-session torch device-to-device copy of the same bytes.

Traffic of one call: (1 + G) * N * batch * sizeof(T) (the input read once, G outputs written).  Per case: warm-up, then
the median of --iters per-iteration HIP event pairs.  One JSON line per case.
    python tools/bench_automorphism.py [--iters 100] [--out profiles/automorphism_bench.jsonl]"""
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

PEAK_BPS = 8e12  # MI355X HBM3E, datasheet
X_N_plus = 0


def median_ms(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    shapes = [  # name, bits, logn, batch, G, moduli
        ("C2", 64, 16, 1024, 1, 1),
        ("C5", 64, 16, 512, 1, 8),
        ("C4", 32, 14, 8192, 1, 1),
        ("fhe_G1", 64, 16, 32, 1, 1),
        ("fhe_G8", 64, 16, 32, 8, 1),
    ]
    lines = []
    for name, bits, logn, batch, G, mc in shapes:
        n = 1 << logn
        dt = torch.int64 if bits == 64 else torch.int32
        wsz = bits // 8
        moduli = [g.Modulus(find_ntt_factors(60 if bits == 64 else 30, logn, skip=i)[0], bits=bits) for i in range(mc)]
        qmin = min(m.value for m in moduli)
        x = torch.randint(0, qmin, (batch * n,), dtype=dt, device=dev)
        out = torch.empty(G * batch * n, dtype=dt, device=dev)
        ks = [g.galois_element_for_rotation(r, logn) for r in range(1, G)] + [g.galois_element_for_conjugation(logn)]
        mods = g.modulus_array_to_device(moduli, bits) if mc > 1 else moduli[0]
        traffic = (1 + G) * n * batch * wsz
        # yardstick: a copy that moves the same bytes (reads half of them, writes the other half)
        src = torch.randint(0, 1 << 20, (traffic // (2 * wsz),), dtype=dt, device=dev)
        dst = torch.empty_like(src)
        res = {"case": name, "dtype": "u%d" % bits, "logN": logn, "batch": batch, "G": G, "moduli": mc,
               "traffic_bytes": traffic}
        res["copy_ms"] = median_ms(lambda: dst.copy_(src), args.iters)
        res["ntt_ms"] = median_ms(lambda: g.GPU_Automorphism_NTT(x, out, ks, logn, X_N_plus, batch), args.iters)
        res["coeff_ms"] = median_ms(lambda: g.GPU_Automorphism(x, out, ks, mods, logn, X_N_plus, batch,
                                                               mod_count=mc), args.iters)
        if G > 1:
            # the same G outputs from G calls with one element each (2G / (1 + G) times the traffic)
            outs = [out[i * batch * n:(i + 1) * batch * n] for i in range(G)]
            res["ntt_ms_G_calls_of_1"] = median_ms(
                lambda: [g.GPU_Automorphism_NTT(x, outs[i], [ks[i]], logn, X_N_plus, batch) for i in range(G)],
                args.iters)
        for key in ("copy", "ntt", "coeff"):
            bps = traffic / (res[key + "_ms"] * 1e-3)
            res[key + "_TBps"] = round(bps / 1e12, 3)
            res[key + "_of_8TBps"] = round(bps / PEAK_BPS, 3)
        res["ntt_over_copy"] = round(res["ntt_ms"] / res["copy_ms"], 3)
        res["coeff_over_copy"] = round(res["coeff_ms"] / res["copy_ms"], 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del x, out, src, dst
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
