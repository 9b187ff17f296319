#!/usr/bin/env python3
"""Device-side key material (include/gpuntt/rns/sampling.cuh and the "Key material" calls of key_switch.cuh), timed at
the shapes of DESIGN.md 3.22: u64 2^16 and u32 2^14, L = 6, K = 2, alpha = 2 (D = 3, M = 8), 16 switching keys.
  sample_uniform   the `a` planes of the 16 keys in place (one call per key: D stacks of M N words, stride 2 M N)
                   and the same words dense in ONE launch (16 enqueues of 10 microseconds each hide the kernel)
  sample_small     the keys' errors, int32[16 D][N], ternary and cbd21, one call; and int32[16 D M][N], as many values
                   as the keys have words, so that the launch does not dominate
  generate_keys    all 16 keys in one call (lift_small, one full-base NTT over 16 D M polynomials, keygen_combine)
Per case: the sampler's words are compared with the host reference first; then warm-up and the median of --iters HIP
event pairs, each around ONE pass over the 16 keys (800 MiB of keys at u64 2^16: every pass writes to HBM).  Bytes per
second count the bytes WRITTEN.  A last line holds the new kernels' register counts as hipcc reports them for gfx950
(-Rpass-analysis=kernel-resource-usage), with their spills.  One JSON line per case.
    python tools/bench_keygen.py [--iters 20] [--out profiles/keygen_bench.jsonl]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import _load_pkg  # noqa: E402
from gpu_utils import find_ntt_factors  # noqa: E402

KEYS = 16


def median_ms(fn, iters, warmup=3):
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


def kernel_name(mangled):
    """_ZN6gpuntt4kern10lift_smallImLi2EEE... -> lift_small<u64, 2>"""
    m = re.match(r"_ZN6gpuntt4kern(\d+)", mangled)
    if not m:
        return mangled
    at = m.end() + int(m.group(1))
    name, rest, args = mangled[m.end():at], mangled[at:], []
    if rest.startswith("I"):
        rest = rest[1:]
        while rest and not rest.startswith("E"):
            lit = re.match(r"Li(\d+)E", rest)
            if lit:
                args.append(lit.group(1))
                rest = rest[lit.end():]
            elif rest[0] in "jm":
                args.append("u32" if rest[0] == "j" else "u64")
                rest = rest[1:]
            else:
                return name + "<" + rest + ">"
    return name + ("<" + ", ".join(args) + ">" if args else "")


def kernel_resources(g):
    """{kernel: {vgprs, sgprs, scratch_bytes, vgpr_spill, sgpr_spill}} of sampling.hip and keygen.hip for gfx950"""
    out = {}
    csrc = g.CSRC
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("sampling", "keygen"):
            r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                                "-I" + csrc, "--offload-arch=gfx950", "-ffp-contract=off",
                                "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, unit + ".hip"), "-o",
                                os.path.join(tmp, unit + ".o")], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            name = None
            for line in r.stderr.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    name = kernel_name(m.group(1))
                    out[name] = {}
                for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                                 ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                 ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
                    m = re.search(pat, line)
                    if m and name:
                        out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    g.load_library()
    dev = "cuda:0"
    lines = []
    for name, bits, logn, L, K, alpha in (("u64_2^16", 64, 16, 6, 2, 2), ("u32_2^14", 32, 14, 6, 2, 2)):
        if args.only and name != args.only:
            continue
        M, n, wsz, D = L + K, 1 << logn, bits // 8, -(-L // alpha)
        dt, npdt = (torch.int64 if bits == 64 else torch.int32), g.np_dtype(bits)
        prms = []
        fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
        for i in range(M):
            prm = g.NTTParameters(logn, g.X_N_plus, bits, find_ntt_factors(59 if bits == 64 else 29, logn, skip=i,
                                                                           clear_of_top=True))
            prms.append(prm)
            fwd[i * n:i * n + prm.root_of_unity_size] = prm.forward_table_device_order
            inv[i * n:i * n + prm.root_of_unity_size] = prm.inverse_table_device_order
        qs = [p.modulus.value for p in prms]
        plan = g.KeySwitchPlan(qs[:L], qs[L:], alpha, logn, g.to_device(fwd), g.to_device(inv), [p.n_inv for p in prms],
                               g.X_N_plus, batch_hint=KEYS * D * M, bits=bits)
        keys = [torch.zeros(D * 2 * M * n, dtype=dt, device=dev) for _ in range(KEYS)]
        errors = torch.zeros(KEYS * D * n, dtype=torch.int32, device=dev)
        s_small = torch.zeros((KEYS + 1) * n, dtype=torch.int32, device=dev)
        g.sample_small(s_small, KEYS + 1, logn, g.TERNARY, 1, 0)
        secrets = torch.zeros((KEYS + 1) * M * n, dtype=dt, device=dev)
        plan.lift_small(s_small, secrets, KEYS + 1, True, True)
        s, s_from = secrets[:M * n], secrets[M * n:]
        scratch = torch.zeros(plan.keygen_scratch_bytes(KEYS), dtype=torch.uint8, device=dev)

        def fill_a():
            for i, k in enumerate(keys):
                g.sample_uniform(k[M * n:], qs, logn, D, 7, i, stack_stride_words=2 * M * n)

        dense = torch.zeros(KEYS * D * M * n, dtype=dt, device=dev)
        many = torch.zeros(KEYS * D * M * n, dtype=torch.int32, device=dev)

        def fill_dense():  # the same words in ONE launch: the kernel without 16 enqueues around it
            g.sample_uniform(dense, qs, logn, KEYS * D, 7, 0)

        def fill_errors(dist):
            g.sample_small(errors, KEYS * D, logn, dist, 9, 0)

        def fill_many(dist):  # as many small values as the keys have words, one launch
            g.sample_small(many, KEYS * D * M, logn, dist, 9, 0)

        def generate():
            plan.generate_keys(s, s_from, errors, keys, scratch)

        fill_a()
        fill_errors(g.CBD21)
        torch.cuda.synchronize()
        ref = g.sample_reference_uniform(qs, logn, D, 7, 3, stack_stride_words=2 * M * n, bits=bits)
        got = g.to_host(keys[3][M * n:])
        same_a = all(np.array_equal(got[d * 2 * M * n:][:M * n], ref[d * 2 * M * n:][:M * n]) for d in range(D))
        same_e = bool(np.array_equal(g.to_host(errors, signed=True), g.sample_reference_small(KEYS * D, logn, g.CBD21, 9, 0)))
        with g.launch_log() as log:
            generate()
        torch.cuda.synchronize()
        a_bytes, e_bytes, key_bytes = KEYS * D * M * n * wsz, KEYS * D * n * 4, KEYS * D * M * n * wsz
        t_a = median_ms(fill_a, args.iters)
        t_d = median_ms(fill_dense, args.iters)
        t_mt = median_ms(lambda: fill_many(g.TERNARY), args.iters)
        t_mc = median_ms(lambda: fill_many(g.CBD21), args.iters)
        t_t = median_ms(lambda: fill_errors(g.TERNARY), args.iters)
        t_c = median_ms(lambda: fill_errors(g.CBD21), args.iters)
        t_g = median_ms(generate, args.iters)
        gbs = lambda b, ms: round(b / ms / 1e6, 1)
        rec = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K": K, "alpha": alpha, "keys": KEYS,
               "key_MiB": round(2 * key_bytes / KEYS / 2**20, 1), "iters": args.iters,
               "sample_uniform_matches_host_reference": bool(same_a), "sample_small_matches_host_reference": same_e,
               "sample_uniform_ms": round(t_a, 4), "sample_uniform_written_GBps": gbs(a_bytes, t_a),
               "sample_uniform_one_launch_ms": round(t_d, 4), "sample_uniform_one_launch_written_GBps": gbs(a_bytes, t_d),
               "sample_small_ternary_key_sized_ms": round(t_mt, 4),
               "sample_small_ternary_key_sized_written_GBps": gbs(KEYS * D * M * n * 4, t_mt),
               "sample_small_cbd21_key_sized_ms": round(t_mc, 4),
               "sample_small_cbd21_key_sized_written_GBps": gbs(KEYS * D * M * n * 4, t_mc),
               "sample_small_ternary_ms": round(t_t, 4), "sample_small_ternary_written_GBps": gbs(e_bytes, t_t),
               "sample_small_cbd21_ms": round(t_c, 4), "sample_small_cbd21_written_GBps": gbs(e_bytes, t_c),
               "generate_keys_ms": round(t_g, 4), "generate_keys_written_GBps": gbs(key_bytes, t_g),
               "generate_keys_launches": [k.split(":")[0] for k in log.kernels]}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del keys, secrets, scratch, dense, many
    rec = {"case": "kernel_resources_gfx950", "kernels": kernel_resources(g)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
