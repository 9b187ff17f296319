"""Shared by the tests of KeySwitchPlan's rescaling calls (include/gpuntt/rns/key_switch.cuh, "Rescaling"): the host
emulator of csrc/rescale.hip, and the calls as COMPOSITIONS of the calls that existed before them -- q-base and full-base
InnerProductPlan.multiply_accumulate, KeySwitchPlan.decompose, GPU_INTT_Inplace over the full base,
BaseConvPlan.convert_and_divide on gathered dense copies and GPU_NTT_Inplace over the kept limbs.  The split of a stack
into {dropped q, p} -> {kept q} is restated here: with L' = L - R, limbs L' .. of a stack are the input base, limbs
0 .. L' - 1 the second operand and the output base."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_baseconv = {}


def run_emulator(tmp_path):
    """cut the kern namespace out of csrc/rescale.hip, build tests/cpp/emulate_rescale.cpp around it for the HOST with
    AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and run
    it; asserts that the program ends with ALL OK and returns what it printed"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "rescale.hip")).read()
    first = text.index("        // grid: x = s * tiles + tile, y = i < R")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_rescale")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_rescale.cpp"), "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def baseconv_plan(g, in_moduli, out_moduli, bits):
    key = (bits, tuple(in_moduli), tuple(out_moduli))
    if key not in _baseconv:
        _baseconv[key] = g.BaseConvPlan(list(in_moduli), list(out_moduli), bits=bits)
    return _baseconv[key]


def dense_divide(g, moduli, keep, x, stacks, n_power, bits):
    """x: a device tensor T[stacks][len(moduli)][N].  Gathers limbs keep .. (the input base) and limbs 0 .. keep - 1 (the
    second operand) into dense copies and returns BaseConvPlan.convert_and_divide of them, centred: T[stacks][keep][N]"""
    from hoisted_utils import filled
    n, limbs = 1 << n_power, len(moduli)
    v = x.view(stacks, limbs, n)
    dropped, kept = v[:, keep:, :].contiguous().view(-1), v[:, :keep, :].contiguous().view(-1)
    out = filled(bits, stacks * keep * n)
    baseconv_plan(g, moduli[keep:], moduli[:keep], bits).convert_and_divide(dropped, kept, out, n_power, stacks, g.CENTRED)
    return out


def composition_rescale(g, plan, st, x, stacks, ntt_form):
    """rescale through GPU_INTT -> gathers -> convert_and_divide -> GPU_NTT on the sub-ring; x holds residues"""
    import torch
    bits, n_power, L, R = plan.bits, plan.n_power, plan.q_count, plan.rescale_limbs
    poly = st["poly"]
    coeff = x.clone()
    if ntt_form:
        cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly,
                                        mod_inverse=st["d_ninv"])
        g.GPU_INTT_Inplace(coeff, st["inv"], st["mods"], cfg_i, stacks * L, L)
    out = dense_divide(g, st["moduli"][:L], L - R, coeff, stacks, n_power, bits)
    if ntt_form:
        cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, stacks * (L - R), L - R)
    torch.cuda.synchronize()
    return out


def tail_rescale(g, plan, st, acc, stacks, output_ntt):
    """acc T[stacks][M][N], NTT form: the full-base GPU_INTT, convert_and_divide by P and the dropped primes, GPU_NTT
    over the kept limbs"""
    import torch
    bits, n_power, L, M, R = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.rescale_limbs
    poly = st["poly"]
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
    g.GPU_INTT_Inplace(acc, st["inv"], st["mods"], cfg_i, stacks * M, M)
    out = dense_divide(g, st["moduli"], L - R, acc, stacks, n_power, bits)
    if output_ntt:
        cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, stacks * (L - R), L - R)
    torch.cuda.synchronize()
    return out


def composition_relin_rescale(g, plan, st, xs, ys, key, count, output_ntt, key_limbs=None):
    """multiply_relinearize_rescale (one pair) and multiply_relinearize_sum_rescale (several) through the calls that
    existed before them: the q-base inner products d0, d1, d2; decompose(d2); the full-base multiply_accumulate with the
    key; P d_c added by a multiply_accumulate with accumulate=True against a constant operand (P mod q_m on the q-limbs, 0
    on the special ones); then tail_rescale.  xs, ys: lists of device tensors of any words, read modulo q_m on the host
    first.  Returns out T[2][count][L - R][N]"""
    import torch
    from hoisted_sum_utils import inner_plan
    from hoisted_utils import filled
    from relin_utils import q_inner_plan
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n, qs = 1 << n_power, st["moduli"]
    dt = g.np_dtype(bits)
    qv = np.array(qs[:L], dtype=dt)[None, None, :, None]
    reduced = {}

    def red(t):
        if t.data_ptr() not in reduced:
            reduced[t.data_ptr()] = g.to_device((g.to_host(t).reshape(2, count, L, n) % qv).reshape(-1)).view(2, count, L, n)
        return reduced[t.data_ptr()]
    xr, yr = [red(t) for t in xs], [red(t) for t in ys]
    qinner = q_inner_plan(g, qs[:L], bits)
    d = filled(bits, 3 * count * L * n).view(3, count, L, n)
    for r in range(count):
        x0, x1 = [x[0, r] for x in xr], [x[1, r] for x in xr]
        y0, y1 = [y[0, r] for y in yr], [y[1, r] for y in yr]
        for c, a, k in ((0, x0, y0), (1, x0 + x1, y1 + y0), (2, x1, y1)):
            qinner.multiply_accumulate(torch.stack(a).reshape(-1), torch.stack(k).reshape(-1), d[c, r].view(-1), n_power,
                                       len(a), 1, 1)
    a = filled(bits, D * count * M * n)
    scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0")
    plan.decompose(d[2].reshape(-1), a, count, True, scratch)
    full = inner_plan(g, st, bits)
    acc = filled(bits, 2 * count * M * n)
    full.multiply_accumulate(a, key, acc, n_power, D, 2, count, False, plan.key_mod_count, key_limbs)
    low = torch.zeros((2, count, M, n), dtype=d.dtype, device="cuda:0")  # d_c on the q-limbs, 0 on the special ones
    low[:, :, :L, :] = d[:2]
    P = math.prod(qs[L:])
    const = np.zeros((M, n), dtype=dt)
    for m in range(L):
        const[m, :] = P % qs[m]
    full.multiply_accumulate(low.view(-1), g.to_device(const.reshape(-1)), acc, n_power, 1, 1, 2 * count, True)
    return tail_rescale(g, plan, st, acc, 2 * count, output_ntt)


def composition_sum_rescale(g, plan, st, a, c0, keys, elts, weights, count, output_ntt, key_limbs=None):
    """rotate_hoisted_sum_rescale through the calls that existed before it: hoisted_sum_utils.composition_sum's steps up
    to the weighted accumulators, then tail_rescale.  Returns out T[2][count][L - R][N]"""
    import torch
    from hoisted_sum_utils import inner_plan
    from hoisted_utils import device_words, filled
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n, G, poly, qs = 1 << n_power, len(elts), st["poly"], st["moduli"]
    dt = g.np_dtype(bits)
    inner = inner_plan(g, st, bits)
    a_rot = filled(bits, G * D * count * M * n)
    g.GPU_Automorphism_NTT(a, a_rot, elts, n_power, poly, D * count * M)
    a_rot = a_rot.view(G, -1)
    u = filled(bits, G * 2 * count * M * n).view(G, 2, count, M, n)
    for i in range(G):
        inner.multiply_accumulate(a_rot[i], keys[i], u[i].view(-1), n_power, D, 2, count, False, plan.key_mod_count,
                                  key_limbs)
    if c0 is not None:
        P = math.prod(qs[L:])
        red = g.to_host(c0).reshape(count, L, n) % np.array(qs[:L], dtype=dt)[None, :, None]
        scaled = np.stack([red[:, m, :].astype(object) * (P % qs[m]) % qs[m] for m in range(L)], axis=1)
        pc0 = device_words(g, np.ascontiguousarray(scaled.astype(np.uint64).astype(dt).reshape(-1)))
        c0_rot = filled(bits, G * count * L * n)
        g.GPU_Automorphism_NTT(pc0, c0_rot, elts, n_power, poly, count * L)
        c0_rot = c0_rot.view(G, count, L, n)
        qt = g.to_device(np.array(qs[:L], dtype=dt)).view(1, 1, L, 1)
        s = u[:, 0, :, :L, :] + c0_rot  # both below q < 2^(W-2): no wrap in the signed type
        u[:, 0, :, :L, :] = torch.where(s >= qt, s - qt, s)
    wkey = np.ones((G, M, n), dtype=dt)
    for i in range(G):
        if weights is not None and weights[i] is not None:
            wkey[i] = g.to_host(weights[i]).reshape(-1)[:M * n].reshape(M, n) % np.array(qs, dtype=dt)[:, None]
    acc = filled(bits, 2 * count * M * n)
    inner.multiply_accumulate(u.view(-1), g.to_device(wkey.reshape(-1)), acc, n_power, G, 1, 2 * count)
    return tail_rescale(g, plan, st, acc, 2 * count, output_ntt)
