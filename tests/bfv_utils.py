"""Shared by the tests of BfvMultiplyPlan (include/gpuntt/rns/bfv_multiply.cuh): the smallest auxiliary base, plan
construction, random operands, the host emulator of csrc/bfv_multiply.hip, and the three calls as COMPOSITIONS of the
public calls that existed before them on the same device data -- BaseConvPlan.convert / convert_and_divide on gathered
dense copies, operator_gpu's multiplication, GPU_NTT / GPU_INTT over the q-base and the full base and
InnerProductPlan.multiply_accumulate per input and tensor term."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_baseconv, _inner = {}, {}


def aux_count(moduli, L, t, n):
    """the smallest K with moduli[L] ... moduli[L + K - 1] >= 2 t n Q, Q = moduli[0] ... moduli[L - 1]"""
    need, B = 2 * t * n * math.prod(moduli[:L]), 1
    for K in range(1, len(moduli) - L + 1):
        B *= moduli[L + K - 1]
        if B >= need:
            return K
    raise ValueError("%d moduli do not hold an auxiliary base for L = %d" % (len(moduli), L))


def run_emulator(tmp_path, job):
    """cut the kern namespace out of csrc/bfv_multiply.hip, build tests/cpp/emulate_bfv.cpp around it for the HOST with
    AddressSanitizer and UBSan (a stand-alone program, one thread per lane; a plain clang++, nothing preloaded) and run
    it on the job file; returns the path of what it wrote"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "bfv_multiply.hip")).read()
    first = text.index("        extern __shared__ __align__(16) unsigned char bfv_smem[];")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_bfv")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_bfv.cpp"), "-o", exe], timeout=300)
    out = str(tmp_path / "result.bin")
    r = subprocess.run([exe, str(job), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return out


def make_plan(g, st, L, t, n_power, bits, **kw):
    """st: hoisted_utils.Ring.sub() of the full base, the q-base first"""
    return g.BfvMultiplyPlan(st["moduli"][:L], st["moduli"][L:], t, n_power, st["fwd"], st["inv"], st["n_inv"],
                             st["poly"], bits=bits, **kw)


def bfv_scratch(plan, count):
    import torch
    return torch.zeros(max(256, plan.scratch_bytes(count)), dtype=torch.uint8, device="cuda:0")


def baseconv_plan(g, in_moduli, out_moduli, bits):
    key = (bits, tuple(in_moduli), tuple(out_moduli))
    if key not in _baseconv:
        _baseconv[key] = g.BaseConvPlan(list(in_moduli), list(out_moduli), bits=bits)
    return _baseconv[key]


def inner_plan(g, moduli, bits):
    key = (bits, tuple(moduli))
    if key not in _inner:
        _inner[key] = g.InnerProductPlan(list(moduli), bits=bits)
    return _inner[key]


def reduced(g, x, moduli, n, bits):
    """a device tensor T[...][len(moduli)][N] of any words -> the same words modulo their limb's modulus (numpy's exact
    unsigned % on the host: the calls of the composition are only defined on residues)"""
    dt = g.np_dtype(bits)
    h = g.to_host(x).reshape(-1, len(moduli), n) % np.array(moduli, dtype=dt)[None, :, None]
    return g.to_device(np.ascontiguousarray(h.reshape(-1)))


def composition_extend(g, moduli, L, x, stacks, n_power, bits):
    """x T[stacks][L][N], residues: the q-limbs as they are beside BaseConvPlan({q} -> {b}).convert, centred"""
    import torch
    from hoisted_utils import filled
    n, K = 1 << n_power, len(moduli) - L
    conv = filled(bits, stacks * K * n)
    baseconv_plan(g, moduli[:L], moduli[L:], bits).convert(x, conv, n_power, stacks, g.CENTRED)
    return torch.cat((x.view(stacks, L, n), conv.view(stacks, K, n)), dim=1).contiguous().view(-1)


def composition_scale_round(g, moduli, L, t, full, stacks, n_power, bits):
    """full T[stacks][M][N], residues: operator_gpu's multiplication by t mod m_m per limb, convert_and_divide of the
    gathered q-limbs and b-limbs, convert of the result; returns out T[stacks][L][N]"""
    import torch
    from hoisted_utils import filled
    n, M = 1 << n_power, len(moduli)
    K, dt = M - L, g.np_dtype(bits)
    v = full.view(stacks, M, n)
    s = torch.empty_like(v)
    for m, q in enumerate(moduli):
        tq = g.to_device(np.full(stacks * n, t % q, dtype=dt))
        s[:, m, :] = g.operator_gpu(2, v[:, m, :].contiguous().view(-1), tq, g.Modulus(q, bits=bits)).view(stacks, n)
    sq, sb = s[:, :L, :].contiguous().view(-1), s[:, L:, :].contiguous().view(-1)
    r = filled(bits, stacks * K * n)
    baseconv_plan(g, moduli[:L], moduli[L:], bits).convert_and_divide(sq, sb, r, n_power, stacks, g.CENTRED)
    out = filled(bits, stacks * L * n)
    baseconv_plan(g, moduli[L:], moduli[:L], bits).convert(r, out, n_power, stacks, g.CENTRED)
    torch.cuda.synchronize()
    return out


def composition_multiply(g, st, L, t, x, y, count, input_ntt, output_ntt, n_power, bits):
    """the seven steps of multiply through the calls that existed before it; x, y: device tensors T[2][count][L][N] of
    any words, read modulo q_m on the host first.  Returns out T[3][count][L][N]"""
    import torch
    from hoisted_utils import filled
    moduli, poly = st["moduli"], st["poly"]
    n, M = 1 << n_power, len(moduli)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
    full = []
    for v in ((x,) if y is x else (x, y)):
        c = reduced(g, v, moduli[:L], n, bits)
        if input_ntt:
            g.GPU_INTT_Inplace(c, st["inv"], st["mods"], cfg_i, 2 * count * L, L)
        e = composition_extend(g, moduli, L, c, 2 * count, n_power, bits)
        g.GPU_NTT_Inplace(e, st["fwd"], st["mods"], cfg_f, 2 * count * M, M)
        full.append(e.view(2, count, M, n))
    xe, ye = full[0], full[-1]
    inner = inner_plan(g, moduli, bits)
    d = filled(bits, 3 * count * M * n).view(3, count, M, n)
    for r in range(count):  # the key operand is shared by all inputs: one call per input and term, gathers for d1
        inner.multiply_accumulate(xe[0, r].reshape(-1), ye[0, r].reshape(-1), d[0, r].view(-1), n_power, 1, 1, 1)
        inner.multiply_accumulate(torch.stack((xe[0, r], xe[1, r])).reshape(-1),
                                  torch.stack((ye[1, r], ye[0, r])).reshape(-1), d[1, r].view(-1), n_power, 2, 1, 1)
        inner.multiply_accumulate(xe[1, r].reshape(-1), ye[1, r].reshape(-1), d[2, r].view(-1), n_power, 1, 1, 1)
    d = d.view(-1)
    g.GPU_INTT_Inplace(d, st["inv"], st["mods"], cfg_i, 3 * count * M, M)
    out = composition_scale_round(g, moduli, L, t, d, 3 * count, n_power, bits)
    if output_ntt:
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, 3 * count * L, L)
    torch.cuda.synchronize()
    return out


def operands(g, rng, bits, moduli, L, count, n, residues=False):
    """x, y T[2][count][L][N] of arbitrary words (0, 2^W - 1, q - 1 and q planted); residues: the same words modulo
    q_m -- what the NTT-form entry of multiply takes, whose first step is a transform"""
    from hoisted_utils import any_words, device_words
    x, y = (device_words(g, any_words(g, rng, bits, 2 * count * L * n, moduli[:L])) for _ in range(2))
    return (reduced(g, x, moduli[:L], n, bits), reduced(g, y, moduli[:L], n, bits)) if residues else (x, y)
