"""Shared by the tests of KeySwitchPlan.lift_small / generate_keys / encrypt_symmetric: the host emulator of lift_small and
keygen_combine (tests/cpp/emulate_keygen.cpp) and the small things both the host and the GPU tests build -- secrets,
errors with the lift's edge values planted, and exact decryption."""
import os
import subprocess

import numpy as np

from keygen_exact import EDGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted_errors(rng, shape, bound=None):
    """int32 values of the whole range (or |v| <= bound), with INT32_MIN, -1, 0 and INT32_MAX planted in every
    polynomial's first and last places when the range is whole"""
    if bound is not None:
        return rng.integers(-bound, bound + 1, size=shape, dtype=np.int64).astype(np.int32)
    x = rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)
    flat = x.reshape(-1, shape[-1])
    for p in range(flat.shape[0]):
        for i, v in enumerate(EDGES):
            flat[p, (i + p) % shape[-1]] = v
    for i, v in enumerate(EDGES):  # every edge is there even when N is below their number (given four words in all)
        flat.reshape(-1)[(i * max(1, flat.size // len(EDGES))) % flat.size] = v
    return x


def emulator_job(cases, arrays):
    """the job file of tests/cpp/emulate_keygen.cpp: cases = [(W, n_power, L, K, alpha, keys, off, moduli)], arrays = per
    case (errors, e, s, s_from, a, ee, ea, msg); signed values travel sign-extended"""
    words = [len(cases)]
    for (W, n_power, L, K, alpha, keys, off, moduli), ops in zip(cases, arrays):
        words += [W, n_power, L, K, alpha, keys, off] + list(moduli)
        for a in ops:
            words += [int(v) & (2**64 - 1) for v in np.asarray(a).reshape(-1)]
    return np.array(words, dtype=np.uint64)


def run_emulator(tmp_path, job):
    """cut the kern namespace out of csrc/keygen.hip, build tests/cpp/emulate_keygen.cpp around it for the HOST with
    AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and run
    it on the job file; returns the words it wrote"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "keygen.hip")).read()
    first = text.index("        // grid: x = p * tiles + tile; small:")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_keygen")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_keygen.cpp"), "-o", exe], timeout=300)
    path = tmp_path / "job.bin"
    job.tofile(str(path))
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(path), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint64), r.stdout
