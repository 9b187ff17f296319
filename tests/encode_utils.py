"""Shared by the BFV batching tests (include/gpuntt/rns/bfv_encode.cuh; KeySwitchPlan.lift_centred / multiply_plain): the
host emulator of the three kernels (tests/cpp/emulate_bfv_encode.cpp), plaintext moduli with their tables, and the
encoder of one (bits, n_power, t)."""
import os
import subprocess

import numpy as np

from encode_exact import plain_factors
from gpu_utils import MergeCase, distinct_factors_scaled, find_ntt_factors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def widest_plain(bits, n_power):
    """the widest NTT prime Modulus<T> takes for that word (bits - 2 bits), with its roots for this ring"""
    return distinct_factors_scaled([bits - 2], n_power)[0]


def plain_for_ring(n_power):
    """(t, omega, psi) of a small plaintext prime with t = 1 mod 2N: 65537 up to 2^15, beyond that the narrowest prime
    find_ntt_factors finds"""
    if n_power <= 15:
        return plain_factors(65537, n_power)
    width = n_power + 2
    while True:
        try:
            return find_ntt_factors(width, n_power)
        except ValueError:
            width += 1


class Encoder:
    """a BfvBatchEncoder with the tables it reads, and the oracle's case for the model"""

    def __init__(self, g, bits, n_power, factors, **kw):
        self.case = MergeCase(g, bits, n_power, g.X_N_plus, factors)
        self.t = factors[0]
        self.plan = g.BfvBatchEncoder(self.case.prm.modulus, n_power, self.case.fwd_dev, self.case.inv_dev,
                                      self.case.prm.n_inv, **kw)


def emulator_job(cases, arrays):
    """the job file of tests/cpp/emulate_bfv_encode.cpp: cases = [(W, n_power, L, K, count, off, slices, t, moduli)],
    arrays = per case (values, spectrum, words, ct, pt)"""
    words = [len(cases)]
    for (W, n_power, L, K, count, off, slices, t, moduli), ops in zip(cases, arrays):
        words += [W, n_power, L, K, count, off, slices, t] + list(moduli)
        for a in ops:
            words += [int(v) & (2**64 - 1) for v in np.asarray(a).reshape(-1)]
    return np.array(words, dtype=np.uint64)


def run_emulator(tmp_path, job):
    """cut the kern namespaces out of csrc/keygen.hip and csrc/bfv_encode.hip, build tests/cpp/emulate_bfv_encode.cpp
    around them for the HOST with AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain
    clang++, nothing preloaded) and run it on the job file; returns the words it wrote"""
    csrc = os.path.join(ROOT, "gpu-ntt_amd", "csrc")
    for name, source, start in (("kernel_extract.inc", "keygen.hip", "        // grid: x = p * tiles + tile; small:"),
                                ("permute_extract.inc", "bfv_encode.hip", "        // grid: x = column tile, y = batch")):
        text = open(os.path.join(csrc, source)).read()
        (tmp_path / name).write_text(text[text.index(start):text.index("    } // namespace kern")])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_bfv_encode")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(cpp, "emulate_bfv_encode.cpp"), "-o", exe], timeout=300)
    path = tmp_path / "job.bin"
    job.tofile(str(path))
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(path), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint64), r.stdout
