"""Shared by the tests of KeySwitchPlan.multiply_relinearize_sum (include/gpuntt/rns/key_switch.cuh): random operands and
the DEFINITION of the call as a composition of the calls that existed before it -- per input three q-base
InnerProductPlan.multiply_accumulate calls over gathered polynomials (D = T for d0 and d2, D = 2 T for d1),
KeySwitchPlan.apply on the top term, GPU_INTT_Inplace and the two additions modulo q_m."""
import numpy as np

from hoisted_utils import any_words, canonical_key, device_words, filled
from relin_utils import q_inner_plan


def relin_sum_operands(g, plan, st, rng, count, terms, km_moduli=None, offset=0):
    """xs, ys: `terms` tensors T[2][count][L][N] each, of arbitrary words (0, 2^W - 1, q - 1 and q planted), and a
    canonical key"""
    bits, n, L, D = plan.bits, 1 << plan.n_power, plan.q_count, plan.digits
    def one():
        return device_words(g, any_words(g, rng, bits, 2 * count * L * n, st["moduli"][:L]), offset)
    xs, ys = [one() for _ in range(terms)], [one() for _ in range(terms)]
    km = st["moduli"] if km_moduli is None else km_moduli
    key = device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset)
    return xs, ys, key


def composition_relin_sum(g, plan, st, xs, ys, key, count, output_ntt):
    """multiply_relinearize_sum's definition through the calls that existed before it; returns out T[2][count][L][N].
    xs, ys: lists of device tensors, key a device tensor.  The operands may hold any words: they are read modulo q_m,
    done here on the host with numpy's exact unsigned % before anything else."""
    import torch
    bits, n_power, L = plan.bits, plan.n_power, plan.q_count
    n, poly, qs = 1 << n_power, st["poly"], st["moduli"][:L]
    T = len(xs)
    assert T == len(ys) and T >= 1
    dt = g.np_dtype(bits)
    qv = np.array(qs, dtype=dt)[None, None, :, None]
    reduced = {}

    def red(t):
        if t.data_ptr() not in reduced:
            reduced[t.data_ptr()] = g.to_device((g.to_host(t).reshape(2, count, L, n) % qv).reshape(-1)).view(2, count, L, n)
        return reduced[t.data_ptr()]
    xr, yr = [red(t) for t in xs], [red(t) for t in ys]
    inner = q_inner_plan(g, qs, bits)
    d = filled(bits, 3 * count * L * n).view(3, count, L, n)
    for r in range(count):  # the key operand is shared by all inputs: one call per input and tensor term
        x0 = [x[0, r] for x in xr]
        x1 = [x[1, r] for x in xr]
        y0 = [y[0, r] for y in yr]
        y1 = [y[1, r] for y in yr]
        for c, a, k in ((0, x0, y0), (1, x0 + x1, y1 + y0), (2, x1, y1)):
            inner.multiply_accumulate(torch.stack(a).reshape(-1), torch.stack(k).reshape(-1), d[c, r].view(-1), n_power,
                                      len(a), 1, 1)
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
