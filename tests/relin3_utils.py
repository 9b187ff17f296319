"""Shared by the tests of KeySwitchPlan.mod_down_add, KeySwitchPlan.relinearize (include/gpuntt/rns/key_switch.cuh) and
BfvMultiplyPlan.multiply_relinearize (include/gpuntt/rns/bfv_multiply.cuh): one ring that supplies the q-base, the
auxiliary base {q, b} and the key-switching base {q, p}; the three calls as COMPOSITIONS of the public calls that existed
before them on the same device data -- mod_down, apply, multiply, the q-base transforms and operator_gpu's modular
addition; and the host emulator of inner_product_seeded and mod_down_add."""
import os
import subprocess

import numpy as np

from bfv_utils import aux_count, composition_multiply, reduced
from hoisted_utils import any_words, canonical_key, device_words, filled, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADD = 0  # operator_gpu's modular addition


def bases(g, bits, n_power, L, t, K_p=2, poly=None, widths=None):
    """(ring, {q, b} stack, {q, p} stack, K_b): the ring's first L primes, the smallest auxiliary base behind them
    (bfv_utils.aux_count) and K_p special primes behind that"""
    full = ring(g, bits, n_power, M=2 * L + 4 + K_p, poly=poly, widths=widths)
    K_b = aux_count(full.moduli[:2 * L + 4], L, t, 1 << n_power)
    q = list(range(L))
    return full, full.sub(q + list(range(L, L + K_b))), full.sub(q + list(range(L + K_b, L + K_b + K_p))), K_b


def add_mod(g, a, b, moduli, n, bits):
    """(a + b) mod q_m per limb through operator_gpu, a and b T[...][len(moduli)][N] of residues; returns a new tensor"""
    import torch
    L = len(moduli)
    va, vb = a.view(-1, L, n), b.view(-1, L, n)
    out = torch.empty_like(va)
    for m, q in enumerate(moduli):
        out[:, m, :] = g.operator_gpu(ADD, va[:, m, :].contiguous().view(-1), vb[:, m, :].contiguous().view(-1),
                                      g.Modulus(q, bits=bits)).view(-1, n)
    return out.view(-1)


def composition_mod_down_add(g, plan, st, x, addend, stacks):
    """mod_down, then the addend -- read modulo q_j on the host first -- added through operator_gpu"""
    import torch
    bits, n, L = plan.bits, 1 << plan.n_power, plan.q_count
    down = filled(bits, stacks * L * n)
    plan.mod_down(x, down, stacks)
    out = add_mod(g, down, reduced(g, addend, st["moduli"][:L], n, bits), st["moduli"][:L], n, bits)
    torch.cuda.synchronize()
    return out


def composition_relinearize(g, plan, st, c01, c2, key, count, input_ntt, output_ntt):
    """relinearize's definition: apply on c2, and c01 -- read modulo q_m on the host, brought to the output's form by the
    q-base transform when the forms differ -- added through operator_gpu.  Returns out T[2][count][L][N]"""
    import torch
    bits, n_power, L = plan.bits, plan.n_power, plan.q_count
    n, poly, qs = 1 << n_power, st["poly"], st["moduli"][:L]
    k = filled(bits, 2 * count * L * n)
    scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0")
    plan.apply(c2, key, k, count, 2, input_ntt, output_ntt, scratch)
    low = reduced(g, c01, qs, n, bits)
    if input_ntt and not output_ntt:
        cfg = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
        g.GPU_INTT_Inplace(low, st["inv"], st["mods"], cfg, 2 * count * L, L)
    elif output_ntt and not input_ntt:
        cfg = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
        g.GPU_NTT_Inplace(low, st["fwd"], st["mods"], cfg, 2 * count * L, L)
    out = add_mod(g, k, low, qs, n, bits)
    torch.cuda.synchronize()
    return out


def composition_bfv(g, ks, st_b, st_p, t, x, y, key, count, input_ntt, output_ntt):
    """BfvMultiplyPlan.multiply_relinearize's definition: multiply(output_ntt = false) through bfv_utils' composition,
    then relinearize's.  Returns out T[2][count][L][N]"""
    L, n = ks.q_count, 1 << ks.n_power
    m = composition_multiply(g, st_b, L, t, x, y, count, input_ntt, False, ks.n_power, ks.bits)
    low, top = m[:2 * count * L * n], m[2 * count * L * n:]
    return composition_relinearize(g, ks, st_p, low, top, key, count, False, output_ntt)


def relin3_operands(g, plan, st, rng, count, input_ntt, km_moduli=None, offset=0):
    """one contiguous T[3][count][L][N] -- c01 of any words (0, 2^W - 1, q - 1 and q planted); c2 of any words in
    coefficient form, of residues in NTT form -- and a canonical key"""
    bits, n, L, D = plan.bits, 1 << plan.n_power, plan.q_count, plan.digits
    qs = st["moduli"][:L]
    ct = device_words(g, any_words(g, rng, bits, 3 * count * L * n, qs), offset)
    if input_ntt:
        ct[2 * count * L * n:] = reduced(g, ct[2 * count * L * n:], qs, n, bits)
    km = st["moduli"] if km_moduli is None else km_moduli
    key = device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset)
    return ct, key


def emulator_job(cases, arrays):
    """the job file of tests/cpp/emulate_relin3.cpp: cases = [(W, n_power, L, K, alpha, count, off, split, moduli)],
    arrays = per case the five operand arrays (object or integer words)"""
    words = [len(cases)]
    for (W, n_power, L, K, alpha, count, off, split, moduli), ops in zip(cases, arrays):
        words += [W, n_power, L, K, alpha, count, off, split] + list(moduli)
        for a in ops:
            words += [int(v) for v in np.asarray(a).reshape(-1)]
    return np.array(words, dtype=np.uint64)


def run_emulator(tmp_path, job):
    """cut the kern namespace out of csrc/relinearize.hip, build tests/cpp/emulate_relin3.cpp around it for the HOST with
    AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and run
    it on the job file; returns the words it wrote"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "relinearize.hip")).read()
    first = text.index("        // How inner_product_tensor seeds")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_relin3")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_relin3.cpp"), "-o", exe], timeout=300)
    path = tmp_path / "job.bin"
    job.tofile(str(path))
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(path), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint64), r.stdout
