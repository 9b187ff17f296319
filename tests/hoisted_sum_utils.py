"""Shared by the tests of KeySwitchPlan.rotate_hoisted_sum (include/gpuntt/rns/key_switch.cuh): random weights and the
DEFINITION of the call as a composition of the calls that existed before it -- GPU_Automorphism_NTT,
InnerProductPlan.multiply_accumulate (once per element for u_g, once more over the G stacks with the weights as the
key), GPU_INTT_Inplace, KeySwitchPlan.mod_down and GPU_NTT_Inplace."""
import math

import numpy as np

from hoisted_utils import any_words, device_words, filled

_inner = {}


def inner_plan(g, st, bits):
    """the InnerProductPlan over the plan's full base, one per (bits, moduli)"""
    key = (bits, tuple(st["moduli"]))
    if key not in _inner:
        _inner[key] = g.InnerProductPlan(st["moduli"], bits=bits)
    return _inner[key]


def sum_scratch(plan, count, short=0):
    import torch
    return torch.zeros(plan.hoisted_sum_scratch_bytes(count) - short, dtype=torch.uint8, device="cuda:0")


def make_weights(g, plan, st, rng, G, offset=0):
    """G device tensors T[M][N] of arbitrary words over the full base, with 0, 2^W - 1, q - 1 and q planted"""
    n = 1 << plan.n_power
    return [device_words(g, any_words(g, rng, plan.bits, plan.mod_count * n, st["moduli"]), offset) for _ in range(G)]


def with_nones(weights, drop):
    """the list with entry `drop` (and every 4th after it) replaced by None"""
    return [None if i % 4 == drop % 4 else w for i, w in enumerate(weights)]


def composition_sum(g, plan, st, a, c0, keys, elts, weights, count, output_ntt, key_limbs=None):
    """rotate_hoisted_sum's definition through the calls that existed before it; returns out T[2][count][L][N].
    a, c0, keys: device tensors; weights: None or a list of device tensors / None.  c0 and the weights may hold any
    words: they are read modulo q_m, done here on the host with numpy's exact unsigned % (c0 then times P mod q_m in
    Python integers) before anything else."""
    import torch
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n, G, poly, qs = 1 << n_power, len(elts), st["poly"], st["moduli"]
    dt = g.np_dtype(bits)
    inner = inner_plan(g, st, bits)
    a_rot = filled(bits, G * D * count * M * n)
    g.GPU_Automorphism_NTT(a, a_rot, elts, n_power, poly, D * count * M)
    a_rot = a_rot.view(G, -1)
    u = filled(bits, G * 2 * count * M * n).view(G, 2, count, M, n)  # the G stacks: "digits" of the second product
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
        s = u[:, 0, :, :L, :] + c0_rot  # both below q < 2^(W-2): 2 q - 2 < 2^(W-1), no wrap in the signed type
        u[:, 0, :, :L, :] = torch.where(s >= qt, s - qt, s)
    wkey = np.ones((G, M, n), dtype=dt)  # T[G][1][M][N]; all-ones limbs for null entries
    for i in range(G):
        if weights is not None and weights[i] is not None:
            wkey[i] = g.to_host(weights[i]).reshape(-1)[:M * n].reshape(M, n) % np.array(qs, dtype=dt)[:, None]
    acc = filled(bits, 2 * count * M * n)
    inner.multiply_accumulate(u.view(-1), g.to_device(wkey.reshape(-1)), acc, n_power, G, 1, 2 * count)
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=st["d_ninv"])
    g.GPU_INTT_Inplace(acc, st["inv"], st["mods"], cfg_i, 2 * count * M, M)
    out = filled(bits, 2 * count * L * n)
    plan.mod_down(acc, out, 2 * count)
    if output_ntt:
        cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=poly)
        g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg_f, 2 * count * L, L)
    torch.cuda.synchronize()
    return out

