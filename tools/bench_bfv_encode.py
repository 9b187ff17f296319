#!/usr/bin/env python3
"""BFV batching and plaintext operands (BfvBatchEncoder.encode / decode, KeySwitchPlan.lift_centred / multiply_plain;
DESIGN.md 3.24), timed at u64 2^16 L = 6 (count 1 and 16) and u32 2^14 L = 6 (count 16), K = 2, alpha = 2; t = 65537 at
2^14 and the narrowest prime = 1 mod 2^17 at 2^16:
  encode           bfv_slot_permute (gather, reduced modulo t), then the inverse transform modulo t
  decode           the forward transform modulo t into the scratch, then bfv_slot_permute
  lift_centred     full base, to NTT form (lift_centred and the full-base NTT over count M polynomials)
  multiply_plain   a shared plaintext, and one per ciphertext
Beside each, two yardsticks, neither of which is the new code:
  composed   the same words from what the library offered before: torch indexing with the host-made map, torch
             remainder and subtraction, the existing NTTPlan / lift_small / InnerProductPlan (shared plaintext) /
             operator_gpu per limb (one plaintext per ciphertext)
  copy       a device-to-device copy that moves the same bytes -- the words the call must read plus the words it must
             write, so a copy of half that many bytes -- timed in the same session: the floor
Warm-up, then the median of --iters HIP event pairs.  Reported, not asserted.  A last line (--resources-only prints it
alone, without a GPU) holds the new kernels' register counts as hipcc reports them for gfx950
(-Rpass-analysis=kernel-resource-usage), with their spills.
    python tools/bench_bfv_encode.py [--iters 20] [--no-resources] [--out profiles/bfv_encode_bench.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from __graft_entry__ import _load_pkg  # noqa: E402

NEW_KERNELS = ("bfv_slot_permute", "lift_centred", "multiply_plain")


def kernel_resources(g):
    import bench_keygen
    import re
    import subprocess
    import tempfile
    out, name = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        for source in ("bfv_encode.hip", "keygen.hip"):
            r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                                "-I" + g.CSRC, "--offload-arch=gfx950", "-ffp-contract=off",
                                "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(g.CSRC, source), "-o",
                                os.path.join(tmp, source + ".o")], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            for line in r.stderr.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    name = bench_keygen.kernel_name(m.group(1))
                    name = name if name.split("<")[0] in NEW_KERNELS else None
                    if name:
                        out[name] = {}
                for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                                 ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                 ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
                    m = re.search(pat, line)
                    if m and name:
                        out[name][key] = int(m.group(1))
    return out


def run_cases(g, iters, only):
    import torch
    from bench_keygen import median_ms
    from encode_utils import plain_for_ring
    from gpu_utils import find_ntt_factors
    dev, lines = "cuda:0", []
    for name, bits, logn, L, KP, alpha, counts in (("u64_2^16", 64, 16, 6, 2, 2, (1, 16)),
                                                   ("u32_2^14", 32, 14, 6, 2, 2, (16,))):
        if only and name != only:
            continue
        n, wsz, M = 1 << logn, bits // 8, L + KP
        dt, npdt = (torch.int64 if bits == 64 else torch.int32), g.np_dtype(bits)
        width = 59 if bits == 64 else 29
        prms = [g.NTTParameters(logn, g.X_N_plus, bits, find_ntt_factors(width, logn, skip=i, clear_of_top=True))
                for i in range(M)]
        fwd, inv = np.zeros(M * n, dtype=npdt), np.zeros(M * n, dtype=npdt)
        for k, p in enumerate(prms):
            fwd[k * n:k * n + p.root_of_unity_size] = p.forward_table_device_order
            inv[k * n:k * n + p.root_of_unity_size] = p.inverse_table_device_order
        qp = [p.modulus.value for p in prms]
        ks = g.KeySwitchPlan(qp[:L], qp[L:], alpha, logn, g.to_device(fwd), g.to_device(inv), [p.n_inv for p in prms],
                             g.X_N_plus, batch_hint=max(counts) * M, bits=bits)
        inner = g.InnerProductPlan(qp[:L], bits=bits)
        mods = [g.Modulus(q, bits=bits) for q in qp[:L]]
        tp = g.NTTParameters(logn, g.X_N_plus, bits, plain_for_ring(logn))
        t, up = tp.modulus.value, (tp.modulus.value + 1) >> 1
        t_fwd, t_inv = g.to_device(tp.forward_table_device_order), g.to_device(tp.inverse_table_device_order)
        enc = g.BfvBatchEncoder(tp.modulus, logn, t_fwd, t_inv, tp.n_inv, batch_hint=max(counts))
        plan_f = g.NTTPlan(t_fwd, tp.modulus, logn, g.X_N_plus, g.FORWARD, None, max(counts))
        plan_i = g.NTTPlan(t_inv, tp.modulus, logn, g.X_N_plus, g.INVERSE, tp.n_inv, max(counts))
        to_position, to_slot = (torch.from_numpy(m.astype(np.int64)).to(dev) for m in g.bfv_slot_maps(logn))
        for count in counts:
            values = torch.zeros(count * n, dtype=dt, device=dev)
            g.sample_uniform(values, [t], logn, count, 1, 0)
            plain, back = torch.zeros_like(values), torch.zeros_like(values)
            scratch = torch.zeros(max(256, enc.scratch_bytes(count)), dtype=torch.uint8, device=dev)
            w = scratch.view(dt)[:count * n]
            lifted, lifted2 = (torch.zeros(count * M * n, dtype=dt, device=dev) for _ in range(2))
            ct = torch.zeros(2 * count * L * n, dtype=dt, device=dev)
            g.sample_uniform(ct, qp[:L], logn, 2 * count, 2, 0)
            pt = torch.zeros(count * L * n, dtype=dt, device=dev)
            g.sample_uniform(pt, qp[:L], logn, count, 3, 0)
            out, out2 = torch.zeros_like(ct), torch.zeros_like(ct)

            def composed_encode():
                plain.view(count, n).copy_(torch.remainder(values, t).view(count, n)[:, to_slot])
                plan_i.execute(plain, plain, count)

            def composed_decode():
                plan_f.execute(plain, w, count)
                back.view(count, n).copy_(w.view(count, n)[:, to_position])

            def composed_lift():
                m = torch.remainder(plain, t)
                ks.lift_small(torch.where(m >= up, m - t, m).to(torch.int32), lifted2, count, True, True)

            def composed_shared():
                inner.multiply_accumulate(ct, pt, out2, logn, 1, 1, 2 * count)

            def composed_each():
                a, b, o = ct.view(2, count, L, n), pt.view(count, L, n), out2.view(2, count, L, n)
                for c in range(2):
                    for r in range(count):
                        for i in range(L):
                            o[c, r, i] = g.operator_gpu(2, a[c, r, i], b[r, i], mods[i])

            def floor_ms(nbytes):
                half = max(1, nbytes // 2)
                a = torch.zeros(half, dtype=torch.uint8, device=dev)
                b = torch.zeros(half, dtype=torch.uint8, device=dev)
                ms = median_ms(lambda: b.copy_(a), iters)
                del a, b
                return ms

            cn, ln = count * n * wsz, L * n * wsz
            cases = [
                ("encode", lambda: enc.encode(values, plain, count), composed_encode, 2 * cn + 4 * n),
                ("decode", lambda: enc.decode(plain, back, count, scratch), composed_decode, 2 * cn + 4 * n),
                ("lift_centred", lambda: ks.lift_centred(plain, t, lifted, count, True, True), composed_lift,
                 cn + count * M * n * wsz),
                ("multiply_plain_shared", lambda: ks.multiply_plain(ct, pt, out, count, 1), composed_shared,
                 4 * count * ln + ln),
                ("multiply_plain_each", lambda: ks.multiply_plain(ct, pt, out, count, count), composed_each,
                 5 * count * ln)]
            rec = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K_special": KP, "count": count, "t": t,
                   "iters": iters}
            for label, fn, composed, nbytes in cases:
                with g.launch_log() as log:
                    fn()
                torch.cuda.synchronize()
                ms, cm, fl = median_ms(fn, iters), median_ms(composed, iters), floor_ms(nbytes)
                rec[label + "_ms"] = round(ms, 4)
                rec[label + "_composed_ms"] = round(cm, 4)
                rec[label + "_copy_floor_ms"] = round(fl, 4)
                rec[label + "_composed_over_new"] = round(cm / ms, 2)
                rec[label + "_over_floor"] = round(ms / fl, 2)
                rec[label + "_launches"] = [k.split(":")[0] for k in log.kernels]
            # the composed forms compute the same words
            enc.encode(values, plain, count)
            keep = plain.clone()
            composed_encode()
            same = bool(torch.equal(keep, plain))
            composed_lift()
            ks.lift_centred(plain, t, lifted, count, True, True)
            composed_shared()
            ks.multiply_plain(ct, pt, out, count, 1)
            torch.cuda.synchronize()
            rec["composed_equal"] = same and bool(torch.equal(lifted, lifted2)) and bool(torch.equal(out, out2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del values, plain, back, scratch, lifted, lifted2, ct, pt, out, out2
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="run the named case alone")
    ap.add_argument("--no-resources", action="store_true", help="skip the compile that reports the register counts")
    ap.add_argument("--resources-only", action="store_true", help="only that compile: needs no GPU")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = _load_pkg()
    lines = []
    if not args.resources_only:
        g.load_library()
        lines += run_cases(g, args.iters, args.only)
    if not args.no_resources:
        rec = {"case": "kernel_resources_gfx950", "kernels": kernel_resources(g)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
