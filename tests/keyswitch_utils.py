"""Shared by the hybrid key switching tests (include/gpuntt/rns/key_switch.cuh): the digit partition, ModUp and ModDown
restated in Python integers from the formulas of base_conversion.cuh (numpy object arrays: one Python int per word), CRT
reconstruction and the negacyclic product in Python integers, and the sequence of public calls that apply stands for."""
import math

import numpy as np

from innerprod_utils import from_words

GUARD = 4096  # bytes of 0xA5 on either side of a guarded buffer
# (L, K, alpha): a single digit, D = L, an uneven last digit, alpha above the 16-term chunk, M = 64, L = 63 with one
# special prime
SHAPES = [(1, 1, 1), (3, 1, 1), (5, 2, 2), (8, 3, 3), (4, 4, 4), (40, 24, 20), (63, 1, 1)]


def partition(L, alpha):
    """S_d = [d alpha, min((d + 1) alpha, L)) for d < ceil(L / alpha)"""
    return [range(d * alpha, min((d + 1) * alpha, L)) for d in range(-(-L // alpha))]


def ref_convert(qs, ps, x, bits, centred):
    """base_conversion.cuh, in Python integers: x [L][...] any words -> [K][...]"""
    W, L = bits, len(qs)
    Q = math.prod(qs)
    y = [(x[i] % q) * pow(Q // q, -1, q) % q for i, q in enumerate(qs)]
    v = 0
    if centred:
        z = 0
        for i, q in enumerate(qs):
            b = q.bit_length()
            z = z + ((y[i] * ((1 << (W - 1 + b)) // q)) >> (b - 1))
        v = (z + (1 << (W - 1))) >> W
    out = np.zeros((len(ps),) + x.shape[1:], dtype=object)
    for j, p in enumerate(ps):
        s = 0
        for i in range(L):
            s = s + y[i] * ((Q // qs[i]) % p)
        out[j] = (s - v * (Q % p)) % p
    return out


def ref_mod_up(qs, ps, alpha, x, bits, centred):
    """x [count][L][N] -> a [D][count][M][N]"""
    L, full = len(qs), list(qs) + list(ps)
    M = len(full)
    parts = partition(L, alpha)
    a = np.zeros((len(parts), x.shape[0], M, x.shape[2]), dtype=object)
    for d, S in enumerate(parts):
        rest = [m for m in range(M) if m not in S]
        conv = ref_convert([qs[i] for i in S], [full[m] for m in rest], np.moveaxis(x[:, list(S), :], 1, 0), bits,
                           centred)
        for m in S:
            a[d, :, m, :] = x[:, m, :] % qs[m]
        for j, m in enumerate(rest):
            a[d, :, m, :] = conv[j]
    return a


def ref_mod_down(qs, ps, x, bits):
    """x [stacks][M][N] -> out [stacks][L][N]: ((c_j - conv_j) P^-1) mod q_j, conv centred from the base p"""
    L = len(qs)
    P = math.prod(ps)
    conv = ref_convert(ps, qs, np.moveaxis(x[:, L:, :], 1, 0), bits, True)
    out = np.zeros((x.shape[0], L, x.shape[2]), dtype=object)
    for j, q in enumerate(qs):
        out[:, j, :] = (x[:, j, :] % q - conv[j]) * pow(P, -1, q) % q
    return out


def crt(residues, moduli):
    """residues [len(moduli)][...] -> the integers in [0, prod moduli)"""
    Q = math.prod(moduli)
    s = 0
    for r, q in zip(residues, moduli):
        s = s + r * ((Q // q) * pow(Q // q, -1, q))
    return s % Q


def centre(x, Q):
    """representatives in [-Q/2, Q/2)"""
    return (x + Q // 2) % Q - Q // 2


def negacyclic(a, b):
    """a * b in Z[X] / (X^N + 1), Python integers"""
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                out[i + j] += int(a[i]) * int(b[j])
            else:
                out[i + j - n] -= int(a[i]) * int(b[j])
    return np.array(out, dtype=object)


def planted_input(rng, bits, qs, shape):
    """any words [count][L][N], with 0, q_i - 1 and 2^W - 1 planted"""
    from innerprod_utils import random_words
    top = (1 << bits) - 1
    x = random_words(rng, shape, bits, [0, top] + [q - 1 for q in qs] + [top, 0])
    for i, q in enumerate(qs):  # every limb sees its own extremes
        x[0, i, 0], x[-1, i, -1] = q - 1, top
    return x


def tdtype(bits):
    import torch
    return torch.int64 if bits == 64 else torch.int32


def ones(bits, size, offset=0):
    import torch
    return torch.full((size + offset,), -1, dtype=tdtype(bits), device="cuda:0")[offset:]


def public_sequence(g, plan, inner, st, c_in, key, count, C, input_ntt, output_ntt, km=None, limbs=None):
    """the calls apply stands for, through the existing bindings"""
    import torch
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n = 1 << n_power
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=g.X_N_plus,
                                    mod_inverse=st["d_ninv"])
    coeff = c_in.clone()
    if input_ntt:
        g.GPU_INTT_Inplace(coeff, st["inv"], st["mods"], cfg_i, count * L, L)
    a = ones(bits, D * count * M * n)
    plan.mod_up(coeff, a, count, g.CENTRED)
    g.GPU_NTT_Inplace(a, st["fwd"], st["mods"], cfg_f, D * count * M, M)
    acc = ones(bits, C * count * M * n)
    inner.multiply_accumulate(a, key, acc, n_power, D, C, count, False, km, limbs)
    g.GPU_INTT_Inplace(acc, st["inv"], st["mods"], cfg_i, C * count * M, M)
    out = ones(bits, C * count * L * n)
    plan.mod_down(acc, out, C * count)
    if output_ntt:
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, C * count * L, L)
    torch.cuda.synchronize()
    return out, a


def unmodified(tensors, keep):
    import torch
    assert all(torch.equal(t, k) for t, k in zip(tensors, keep)), "an input was modified"


def column_sample(total, seed):
    """at least 2048 of the `total` = count N columns: the first and the last 64, both sides of every multiple of 2^13,
    2048 seeded random ones"""
    cols = set(range(64)) | set(range(total - 64, total))
    for m in range(1 << 13, total, 1 << 13):
        cols |= {m - 1, m}
    cols |= set(int(c) for c in np.random.default_rng(seed).choice(total, size=2048, replace=False))
    assert len(cols) >= 2048
    return np.array(sorted(cols))


def columns_of(flat, lead, count, rows, n, cols):
    """flat words of a [lead][count][rows][N] -> Python integers [lead][rows][len(cols)]; columns count over count N"""
    x = np.asarray(flat).reshape(lead, count, rows, n).transpose(0, 2, 1, 3).reshape(lead, rows, count * n)
    return from_words(np.ascontiguousarray(x[:, :, cols]), (lead, rows, len(cols)))


def guarded(nbytes):
    """exactly nbytes from the middle of a buffer of 0xA5; returns (the buffer, the view)"""
    import torch
    big = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big.data_ptr() % 256 == 0
    return big, big[GUARD:GUARD + nbytes]


def guards_intact(big):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[-GUARD:] == 0xA5).all())
