"""Shared by the tests of BfvMultiplyPlan.multiply_sum and multiply_relinearize_sum (include/gpuntt/rns/bfv_multiply.cuh):
the host emulator of csrc/bfv_multiply_sum.hip, and the two calls as COMPOSITIONS of the public calls that existed before
them on the same device data -- the q-base and full-base transforms, BaseConvPlan.convert for extend,
InnerProductPlan.multiply_accumulate for the three summed tensor terms (D = terms, 2 * terms, terms), then bfv_utils'
scale_round composition and relin3_utils' relinearize composition."""
import os
import subprocess

import numpy as np

from bfv_utils import composition_extend, composition_scale_round, inner_plan, reduced
from relin3_utils import composition_relinearize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sum_emulator(tmp_path, job):
    """cut the kern namespace out of csrc/bfv_multiply_sum.hip, build tests/cpp/emulate_bfv_sum.cpp around it for the HOST
    with AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and
    run it on the job (an array of 64-bit words); returns (the words it wrote, what it printed)"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "bfv_multiply_sum.hip")).read()
    first = text.index("        // grid: x = r * tiles + tile, y = m < M; e: T[slots]")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_bfv_sum")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_bfv_sum.cpp"), "-o", exe], timeout=300)
    path = tmp_path / "job.bin"
    np.asarray(job, dtype=np.uint64).tofile(str(path))
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(path), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint64), r.stdout


def distinct_tensors(xs, ys):
    """the distinct operand tensors by data pointer, in order of first appearance, and the slots of every term"""
    seen, order, x_slot, y_slot = {}, [], [], []
    for x, y in zip(xs, ys):
        for v, where in ((x, x_slot), (y, y_slot)):
            if v.data_ptr() not in seen:
                seen[v.data_ptr()] = len(order)
                order.append(v)
            where.append(seen[v.data_ptr()])
    return order, x_slot, y_slot


def sum_scratch(plan, count, operands):
    import torch
    return torch.zeros(max(256, plan.sum_scratch_bytes(count, operands)), dtype=torch.uint8, device="cuda:0")


def composition_multiply_sum(g, st, L, t, xs, ys, count, input_ntt, output_ntt, n_power, bits):
    """the definition of multiply_sum through the calls that existed before it; xs, ys: lists of device tensors
    T[2][count][L][N] of any words, read modulo q_m on the host first.  Returns out T[3][count][L][N]"""
    import torch
    from hoisted_utils import filled
    moduli, poly = st["moduli"], st["poly"]
    n, M = 1 << n_power, len(moduli)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
    order, x_slot, y_slot = distinct_tensors(xs, ys)
    full = []
    for v in order:
        c = reduced(g, v, moduli[:L], n, bits)
        if input_ntt:
            g.GPU_INTT_Inplace(c, st["inv"], st["mods"], cfg_i, 2 * count * L, L)
        e = composition_extend(g, moduli, L, c, 2 * count, n_power, bits)
        g.GPU_NTT_Inplace(e, st["fwd"], st["mods"], cfg_f, 2 * count * M, M)
        full.append(e.view(2, count, M, n))
    inner = inner_plan(g, moduli, bits)
    terms = len(xs)
    d = filled(bits, 3 * count * M * n).view(3, count, M, n)
    for r in range(count):  # the key operand is shared by all inputs: one call per input and tensor term, gathered
        def gather(side, comp):
            return torch.stack([full[s][c, r] for s, c in zip(side, comp)]).reshape(-1)
        zeros, ones = [0] * terms, [1] * terms
        inner.multiply_accumulate(gather(x_slot, zeros), gather(y_slot, zeros), d[0, r].view(-1), n_power, terms, 1, 1)
        inner.multiply_accumulate(gather(x_slot + x_slot, zeros + ones), gather(y_slot + y_slot, ones + zeros),
                                  d[1, r].view(-1), n_power, 2 * terms, 1, 1)
        inner.multiply_accumulate(gather(x_slot, ones), gather(y_slot, ones), d[2, r].view(-1), n_power, terms, 1, 1)
    d = d.view(-1)
    g.GPU_INTT_Inplace(d, st["inv"], st["mods"], cfg_i, 3 * count * M, M)
    out = composition_scale_round(g, moduli, L, t, d, 3 * count, n_power, bits)
    if output_ntt:
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, 3 * count * L, L)
    torch.cuda.synchronize()
    return out


def composition_bfv_sum(g, ks, st_b, st_p, t, xs, ys, key, count, input_ntt, output_ntt):
    """multiply_relinearize_sum's definition: multiply_sum(output_ntt = false) through the composition above, then
    relinearize's.  Returns out T[2][count][L][N]"""
    L, n = ks.q_count, 1 << ks.n_power
    m = composition_multiply_sum(g, st_b, L, t, xs, ys, count, input_ntt, False, ks.n_power, ks.bits)
    low, top = m[:2 * count * L * n], m[2 * count * L * n:]
    return composition_relinearize(g, ks, st_p, low, top, key, count, False, output_ntt)
