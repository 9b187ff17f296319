"""Shared by the tests of KeySwitchPlan.linear_transform_bsgs (include/gpuntt/rns/key_switch.cuh): the operand makers and
the DEFINITION of the call as a composition of the calls that existed before it -- GPU_Automorphism_NTT,
InnerProductPlan.multiply_accumulate, GPU_INTT_Inplace / GPU_NTT_Inplace, KeySwitchPlan.mod_down / mod_down_rescale and
KeySwitchPlan.decompose -- with the P c products in Python integers and the modular additions in torch."""
import math

import numpy as np

from hoisted_sum_utils import inner_plan
from hoisted_utils import any_words, canonical_key, device_words, filled


def bsgs_scratch(plan, count, n1, n2, short=0):
    import torch
    return torch.zeros(plan.bsgs_scratch_bytes(count, n1, n2) - short, dtype=torch.uint8, device="cuda:0")


def bsgs_elements(g, n_power, steps, null_at=None):
    """`steps` elements: rotations by 1, -1, 2, ..., the conjugation third and a duplicate of the first fifth; the
    identity at null_at (where the key may be null)"""
    base = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_rotation(-1, n_power),
            g.galois_element_for_conjugation(n_power), g.galois_element_for_rotation(2, n_power),
            g.galois_element_for_rotation(1, n_power)]
    e = (base + [g.galois_element_for_rotation(s, n_power) for s in range(3, steps)])[:steps]
    if null_at is not None:
        e[null_at] = 1
    return e


def bsgs_operands(g, plan, st, rng, count, n1, n2, km_moduli=None, offset=0):
    """a, c0, c1 and n2 x n1 weights of arbitrary words (0, 2^W - 1, q - 1 and q planted), n1 + n2 canonical keys"""
    bits, n = plan.bits, 1 << plan.n_power
    L, M, D = plan.q_count, plan.mod_count, plan.digits
    qs = st["moduli"]
    a = device_words(g, any_words(g, rng, bits, D * count * M * n, qs), offset)
    c0 = device_words(g, any_words(g, rng, bits, count * L * n, qs[:L]), offset)
    c1 = device_words(g, any_words(g, rng, bits, count * L * n, qs[:L]), offset)
    km = qs if km_moduli is None else km_moduli

    def key():
        return device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset)
    bkeys, gkeys = [key() for _ in range(n1)], [key() for _ in range(n2)]
    weights = [[device_words(g, any_words(g, rng, bits, M * n, qs), offset) for _ in range(n1)] for _ in range(n2)]
    return a, c0, c1, bkeys, gkeys, weights


def with_absent(weights, shift):
    """one absent weight in every row with more than one entry, at a column that moves with the row and with `shift`:
    never a whole row"""
    n1 = len(weights[0])
    return [[None if n1 > 1 and b == (gi + shift) % n1 else w for b, w in enumerate(row)]
            for gi, row in enumerate(weights)]


def _add_mod(x, y, qt):
    """(x + y) mod q for canonical residues below 2^(W-2) < 2^(W-1): no wrap in the signed torch type"""
    import torch
    s = x + y
    return torch.where(s >= qt, s - qt, s)


def composition_bsgs(g, plan, st, a, c0, c1, bkeys, belts, gkeys, gelts, weights, count, output_ntt, key_limbs=None,
                     rescale=False):
    """linear_transform_bsgs's DEFINITION (key_switch.cuh) through the calls that existed before it; returns out
    T[2][count][L][N] (L' with rescale).  bkeys / gkeys: lists of device tensors or None (element 1); weights: n2 lists
    of n1 device tensors or None (absent).  c0, c1 and the weights may hold any words: they are read modulo q_m on the
    host with numpy's exact unsigned % (c then times P mod q_m in Python integers) before anything else."""
    import torch
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n, poly, qs = 1 << n_power, st["poly"], st["moduli"]
    n1, n2 = len(belts), len(gelts)
    dt = g.np_dtype(bits)
    inner = inner_plan(g, st, bits)
    P = math.prod(qs[L:])
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
    q_low = g.to_device(np.array(qs[:L], dtype=dt)).view(1, L, 1)
    q_all = g.to_device(np.array(qs, dtype=dt)).view(1, M, 1)

    def scaled(c):  # (P mod q_m) * (c mod q_m) mod q_m: a device tensor T[count][L][N], or None
        if c is None:
            return None
        red = g.to_host(c).reshape(-1)[:count * L * n].reshape(count, L, n) % np.array(qs[:L], dtype=dt)[None, :, None]
        sc = np.stack([red[:, m, :].astype(object) * (P % qs[m]) % qs[m] for m in range(L)], axis=1)
        return device_words(g, np.ascontiguousarray(sc.astype(np.uint64).astype(dt).reshape(-1)))

    def rotated(x, k, polys):
        out = filled(bits, x.numel())
        g.GPU_Automorphism_NTT(x, out, [k], n_power, poly, polys)
        return out

    # 1. the baby accumulators
    pc = [scaled(c0), scaled(c1)]
    u = filled(bits, n1 * 2 * count * M * n, value=0).view(n1, 2, count, M, n)
    for b in range(n1):
        if bkeys[b] is None:
            for c in range(2):
                if pc[c] is not None:
                    u[b, c, :, :L, :] = pc[c].view(count, L, n)
            continue
        a_rot = rotated(a, belts[b], D * count * M)
        inner.multiply_accumulate(a_rot, bkeys[b], u[b].view(-1), n_power, D, 2, count, False, plan.key_mod_count,
                                  key_limbs)
        if pc[0] is not None:
            u[b, 0, :, :L, :] = _add_mod(u[b, 0, :, :L, :], rotated(pc[0], belts[b], count * L).view(count, L, n), q_low)

    # 2. the weighted sums; 3. the giant steps; 4. their sum
    q_mod = np.array(qs, dtype=dt)[:, None]
    acc = None
    for gi in range(n2):
        wkey = np.zeros((n1, M, n), dtype=dt)  # the weights as the key: T[n1][1][M][N]; zero limbs where absent
        for b in range(n1):
            if weights[gi][b] is not None:
                wkey[b] = g.to_host(weights[gi][b]).reshape(-1)[:M * n].reshape(M, n) % q_mod
        v = filled(bits, 2 * count * M * n)
        inner.multiply_accumulate(u.view(-1), g.to_device(wkey.reshape(-1)), v, n_power, n1, 1, 2 * count)
        v = v.view(2, count, M, n)
        if gkeys[gi] is None:
            s = v
        else:
            coeff = v[1].clone().view(-1)
            g.GPU_INTT_Inplace(coeff, st["inv"], st["mods"], cfg_i, count * M, M)
            t = filled(bits, count * L * n)
            plan.mod_down(coeff, t, count)
            a2 = filled(bits, D * count * M * n)
            plan.decompose(t, a2, count, False, None)
            s = filled(bits, 2 * count * M * n)
            inner.multiply_accumulate(rotated(a2, gelts[gi], D * count * M), gkeys[gi], s, n_power, D, 2, count, False,
                                      plan.key_mod_count, key_limbs)
            s = s.view(2, count, M, n)
            s[0] = _add_mod(s[0], rotated(v[0].contiguous().view(-1), gelts[gi], count * M).view(count, M, n), q_all)
        acc = s.clone() if acc is None else _add_mod(acc, s, q_all.view(1, 1, M, 1))

    # the plan's finish over 2 * count stacks
    acc = acc.contiguous().view(-1)
    g.GPU_INTT_Inplace(acc, st["inv"], st["mods"], cfg_i, 2 * count * M, M)
    keep = plan.kept_count if rescale else L
    out = filled(bits, 2 * count * keep * n)
    if rescale:
        plan.mod_down_rescale(acc, out, 2 * count)
    else:
        plan.mod_down(acc, out, 2 * count)
    if output_ntt:
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, 2 * count * keep, keep)
    torch.cuda.synchronize()
    return out
