#!/usr/bin/env python3
"""Decryption and public-key encryption (KeySwitchPlan.phase / encrypt_public, BfvMultiplyPlan.scale_message / decode /
decrypt), timed at u64 2^16 L = 6 (count 1 and 16) and u32 2^14 L = 6 (count 16), K = 2, alpha = 2,
t = 65537, the auxiliary base the smallest that holds 2 t N Q:
  phase            2 and 3 components, NTT form in, coefficient form out (decrypt_phase and the q-base INTT)
  decode           without noise_max, with it (a memset, bfv_decode with one atomicMax per workgroup) and with it in the
                   two-launch form (partial maxima, bfv_decode_merge, no memset)
  decrypt          2 components, NTT form in: phase into the scratch, then decode
  scale_message    to NTT form (bfv_scale_message and the q-base NTT)
  encrypt_public   with a message (lift_small, the q-base NTT over 3 count L polynomials, encrypt_public_combine)
Beside each: a device-to-device copy that moves the same bytes -- the words the call must read plus the words it must
write, so a copy of half that many bytes -- timed in the same session: the floor.  Warm-up, then the median of --iters
HIP event pairs.  Reported, not asserted.  A last line (--resources-only prints it alone, without a GPU) holds the new
kernels' register counts as hipcc reports them for gfx950 (-Rpass-analysis=kernel-resource-usage), with their spills.
    python tools/bench_decrypt.py [--iters 20] [--no-resources] [--out profiles/decrypt_bench.jsonl]"""
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

T_PLAIN = 65537


def kernel_resources(g):
    import bench_keygen
    import re
    import subprocess
    import tempfile
    out, name = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                            "-I" + g.CSRC, "--offload-arch=gfx950", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(g.CSRC, "decrypt.hip"), "-o",
                            os.path.join(tmp, "decrypt.o")], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = bench_keygen.kernel_name(m.group(1))
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
    from gpu_utils import find_ntt_factors
    dev, lines = "cuda:0", []
    for name, bits, logn, L, KP, alpha, counts in (("u64_2^16", 64, 16, 6, 2, 2, (1, 16)),
                                                   ("u32_2^14", 32, 14, 6, 2, 2, (16,))):
        if only and name != only:
            continue
        n, wsz = 1 << logn, bits // 8
        dt, npdt = (torch.int64 if bits == 64 else torch.int32), g.np_dtype(bits)
        width = 59 if bits == 64 else 29
        KB = -(-(1 + T_PLAIN.bit_length() + logn + L * width) // (width - 1))  # B >= 2 t N Q with room
        total = L + KB + KP
        prms = [g.NTTParameters(logn, g.X_N_plus, bits, find_ntt_factors(width, logn, skip=i, clear_of_top=True))
                for i in range(total)]

        def stack(idx):
            fwd, inv = np.zeros(len(idx) * n, dtype=npdt), np.zeros(len(idx) * n, dtype=npdt)
            for k, i in enumerate(idx):
                fwd[k * n:k * n + prms[i].root_of_unity_size] = prms[i].forward_table_device_order
                inv[k * n:k * n + prms[i].root_of_unity_size] = prms[i].inverse_table_device_order
            return ([prms[i].modulus.value for i in idx], g.to_device(fwd), g.to_device(inv),
                    [prms[i].n_inv for i in idx])

        qb, fwd_b, inv_b, ninv_b = stack(list(range(L + KB)))
        qp, fwd_p, inv_p, ninv_p = stack(list(range(L)) + list(range(L + KB, total)))
        M = L + KP
        bfv = g.BfvMultiplyPlan(qb[:L], qb[L:], T_PLAIN, logn, fwd_b, inv_b, ninv_b, g.X_N_plus,
                                batch_hint=max(counts) * L, bits=bits)
        ks = g.KeySwitchPlan(qp[:L], qp[L:], alpha, logn, fwd_p, inv_p, ninv_p, g.X_N_plus,
                             batch_hint=3 * max(counts) * L, bits=bits)
        for count in counts:
            words = count * L * n
            ct = torch.zeros(3 * words, dtype=dt, device=dev)
            g.sample_uniform(ct, qp[:L], logn, 3 * count, 1, 0)
            s = torch.zeros(M * n, dtype=dt, device=dev)
            g.sample_uniform(s, qp, logn, 1, 2, 0)
            ph = torch.zeros(words, dtype=dt, device=dev)
            msg, worst = torch.zeros(count * n, dtype=dt, device=dev), torch.zeros(count, dtype=dt, device=dev)
            plain = torch.zeros(count * n, dtype=dt, device=dev)
            g.sample_uniform(plain, [T_PLAIN], logn, count, 3, 0)
            scaled = torch.zeros(words, dtype=dt, device=dev)
            small = torch.zeros(3 * count * n, dtype=torch.int32, device=dev)
            g.sample_small(small, 3 * count, logn, g.CBD21, 4, 0)
            pk = ct[:2 * L * n].clone()
            out2 = torch.zeros(2 * words, dtype=dt, device=dev)
            d_scr = torch.zeros(max(256, bfv.decrypt_scratch_bytes(count)), dtype=torch.uint8, device=dev)
            e_scr = torch.zeros(max(256, ks.encrypt_public_scratch_bytes(count)), dtype=torch.uint8, device=dev)
            part = torch.zeros(max(256, bfv.decode_partials_bytes(count)), dtype=torch.uint8, device=dev)

            def floor_ms(nbytes):
                half = max(1, nbytes // 2)
                a = torch.zeros(half, dtype=torch.uint8, device=dev)
                b = torch.zeros(half, dtype=torch.uint8, device=dev)
                ms = median_ms(lambda: b.copy_(a), iters)
                del a, b
                return ms

            ln, cn = L * n * wsz, count * n * wsz
            cases = [
                ("phase_2", lambda: ks.phase(ct, s, ph, count, 2, True, False), (2 * count + 1) * ln + count * ln),
                ("phase_3", lambda: ks.phase(ct, s, ph, count, 3, True, False), (3 * count + 1) * ln + count * ln),
                ("decode_noise", lambda: bfv.decode(ph, msg, worst, count), count * ln + cn),
                ("decode_noise_two_launch", lambda: bfv.decode(ph, msg, worst, count, partials=part), count * ln + cn),
                ("decode", lambda: bfv.decode(ph, msg, None, count), count * ln + cn),
                ("decrypt", lambda: bfv.decrypt(ct, ks, s, msg, worst, count, 2, True, d_scr, None),
                 (2 * count + 1) * ln + cn),
                ("scale_message", lambda: bfv.scale_message(plain, scaled, count, True), cn + count * ln),
                ("encrypt_public", lambda: ks.encrypt_public(pk, small, scaled, out2, count, e_scr),
                 2 * ln + 3 * count * n * 4 + count * ln + 2 * count * ln)]
            rec = {"case": name, "dtype": "u%d" % bits, "logN": logn, "L": L, "K_aux": KB, "K_special": KP,
                   "count": count, "t": T_PLAIN, "iters": iters}
            for label, fn, nbytes in cases:
                with g.launch_log() as log:
                    fn()
                torch.cuda.synchronize()
                ms, fl = median_ms(fn, iters), floor_ms(nbytes)
                rec[label + "_ms"] = round(ms, 4)
                rec[label + "_copy_floor_ms"] = round(fl, 4)
                rec[label + "_over_floor"] = round(ms / fl, 2)
                rec[label + "_launches"] = [k.split(":")[0] for k in log.kernels]
            rec["decode_noise_over_decode"] = round(rec["decode_noise_ms"] / rec["decode_ms"], 3)
            rec["decode_noise_two_launch_over_decode"] = round(rec["decode_noise_two_launch_ms"] / rec["decode_ms"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del ct, ph, scaled, out2, d_scr, e_scr
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
