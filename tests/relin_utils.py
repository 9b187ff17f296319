"""Shared by the tests of KeySwitchPlan.multiply_relinearize (include/gpuntt/rns/key_switch.cuh): random operands and the
DEFINITION of the call as a composition of the calls that existed before it -- a q-base
InnerProductPlan.multiply_accumulate per input and tensor term (its "key" operand is shared by all inputs, so the
polynomials of one input are gathered first), KeySwitchPlan.apply on the top term, GPU_INTT_Inplace and the two additions
modulo q_m."""
import numpy as np

from hoisted_utils import any_words, canonical_key, device_words, filled

_inner = {}


def q_inner_plan(g, qs, bits):
    """the InnerProductPlan over the q-base, one per (bits, moduli)"""
    key = (bits, tuple(qs))
    if key not in _inner:
        _inner[key] = g.InnerProductPlan(list(qs), bits=bits)
    return _inner[key]


def relin_scratch(plan, count, short=0):
    import torch
    return torch.zeros(plan.scratch_bytes(count, 2) - short, dtype=torch.uint8, device="cuda:0")


def relin_operands(g, plan, st, rng, count, km_moduli=None, offset=0):
    """x, y T[2][count][L][N] of arbitrary words (0, 2^W - 1, q - 1 and q planted) and a canonical key"""
    bits, n, L, D = plan.bits, 1 << plan.n_power, plan.q_count, plan.digits
    x = device_words(g, any_words(g, rng, bits, 2 * count * L * n, st["moduli"][:L]), offset)
    y = device_words(g, any_words(g, rng, bits, 2 * count * L * n, st["moduli"][:L]), offset)
    km = st["moduli"] if km_moduli is None else km_moduli
    key = device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset)
    return x, y, key


def composition_relin(g, plan, st, x, y, key, count, output_ntt):
    """multiply_relinearize's definition through the calls that existed before it; returns out T[2][count][L][N].
    x, y, key: device tensors.  x and y may hold any words: they are read modulo q_m, done here on the host with numpy's
    exact unsigned % before anything else."""
    import torch
    bits, n_power, L = plan.bits, plan.n_power, plan.q_count
    n, poly, qs = 1 << n_power, st["poly"], st["moduli"][:L]
    dt = g.np_dtype(bits)
    qv = np.array(qs, dtype=dt)[None, None, :, None]
    xr = g.to_device((g.to_host(x).reshape(2, count, L, n) % qv).reshape(-1)).view(2, count, L, n)
    yr = xr if y is x else g.to_device((g.to_host(y).reshape(2, count, L, n) % qv).reshape(-1)).view(2, count, L, n)
    inner = q_inner_plan(g, qs, bits)
    d = filled(bits, 3 * count * L * n).view(3, count, L, n)
    for r in range(count):  # the key operand is shared by all inputs: one call per input and term, gathers for d1
        inner.multiply_accumulate(xr[0, r].reshape(-1), yr[0, r].reshape(-1), d[0, r].view(-1), n_power, 1, 1, 1)
        inner.multiply_accumulate(torch.stack((xr[0, r], xr[1, r])).reshape(-1),
                                  torch.stack((yr[1, r], yr[0, r])).reshape(-1), d[1, r].view(-1), n_power, 2, 1, 1)
        inner.multiply_accumulate(xr[1, r].reshape(-1), yr[1, r].reshape(-1), d[2, r].view(-1), n_power, 1, 1, 1)
    out = filled(bits, 2 * count * L * n).view(2, count, L, n)
    scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0")
    plan.apply(d[2].reshape(-1), key, out.view(-1), count, 2, True, output_ntt, scratch)
    low = d[:2].contiguous()
    if not output_ntt:
        cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly,
                                        mod_inverse=st["d_ninv"])
        g.GPU_INTT_Inplace(low.view(-1), st["inv"], st["mods"], cfg_i, 2 * count * L, L)
    qt = g.to_device(np.array(qs, dtype=dt)).view(1, 1, L, 1)
    s = out + low  # both below q < 2^(W-2): 2 q - 2 < 2^(W-1), no wrap in the signed type
    out = torch.where(s >= qt, s - qt, s)
    torch.cuda.synchronize()
    return out.reshape(-1)
