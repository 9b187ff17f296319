"""Shared by the tests of KeySwitchPlan.phase / encrypt_public and BfvMultiplyPlan.scale_message / decode / decrypt: the
host emulator of csrc/decrypt.hip (tests/cpp/emulate_decrypt.cpp), the inputs decode is probed with -- random, fresh and
the planted half-edges that hit its band -- and the plaintext moduli of the tests."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, t) of the decode checks
PLAIN = {64: [2, 257, 65537, (1 << 31) - 1, (1 << 59) + 1], 32: [2, 257, 65537, (1 << 27) + 1]}


def usable(t, qs, W):
    """2 <= t < 2^(W-2), t below and coprime to every q_i"""
    return 2 <= t < 1 << (W - 2) and all(t < q and math.gcd(t, q) == 1 for q in qs)


def top_plain(qs, W):
    """the largest usable t just below 2^(W-2) (and below the smallest q_i)"""
    t = min(1 << (W - 2), min(qs)) - 1
    while not usable(t, qs, W):
        t -= 1
    return t


def random_x(rng, Q, count):
    """uniform integers in [0, Q) as Python integers"""
    nbytes = (Q.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rng.bytes(nbytes), "little") % Q for _ in range(count)]


def fresh_x(rng, Q, t, count, bound=2000):
    """x = floor((Q m + h) / t) + e with |e| <= bound: what a fresh encryption decrypts from; returns (x, m)"""
    ms = [int(v) for v in rng.integers(0, min(t, 1 << 62), size=count)]
    es = [int(v) for v in rng.integers(-bound, bound + 1, size=count)]
    return [((Q * m + t // 2) // t + e) % Q for m, e in zip(ms, es)], ms


def half_edges(rng, Q, t, count):
    """x = floor(Q (2 k + 1) / (2 t)) + {0, 1}: t x / Q sits at a rounding edge, where decode's band lies"""
    ks = [int(v) for v in rng.integers(0, min(t, 1 << 62), size=count)]
    return [((Q * (2 * k + 1)) // (2 * t) + (i & 1)) % Q for i, k in enumerate(ks)]


def residues(xs, qs):
    """integers -> object array [L][len(xs)]"""
    return np.array([[x % q for x in xs] for q in qs], dtype=object)


def emulator_job(cases, arrays):
    """the job file of tests/cpp/emulate_decrypt.cpp: cases = [(W, n_power, L, count, off, t, moduli)], arrays = per case
    (ct, s, pk, lifted, msg, message, x)"""
    words = [len(cases)]
    for (W, n_power, L, count, off, t, moduli), ops in zip(cases, arrays):
        words += [W, n_power, L, count, off, t] + list(moduli)
        for a in ops:
            words += [int(v) & (2**64 - 1) for v in np.asarray(a).reshape(-1)]
    return np.array(words, dtype=np.uint64)


def run_emulator(tmp_path, job):
    """cut the kern namespace out of csrc/decrypt.hip, build tests/cpp/emulate_decrypt.cpp around it for the HOST with
    AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and run
    it on the job file; returns the words it wrote"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "decrypt.hip")).read()
    first = text.index("        __device__ __forceinline__ void dec_atomic_max(Data32* at")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_decrypt")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_decrypt.cpp"), "-o", exe], timeout=300)
    path = tmp_path / "job.bin"
    job.tofile(str(path))
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(path), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint64), r.stdout
