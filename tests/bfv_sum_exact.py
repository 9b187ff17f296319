"""BfvMultiplyPlan.multiply_sum and multiply_relinearize_sum (include/gpuntt/rns/bfv_multiply.cuh) restated in Python
integers (numpy object arrays: one Python int per word).  No GPU call and none of the library's arithmetic: bfv_exact,
relin3_exact and hoisted_exact are imported, not edited.  Every step is defined word for word, so what these functions
return is compared with array_equal.  Beside the definition: the bound of the header on the difference from `terms`
separate calls."""
import numpy as np

from bfv_exact import exact_extend, exact_scale_round, in_band
from hoisted_exact import transform
from relin3_exact import exact_definition

MAX_TERMS = 32


def slots_of(xs, ys):
    """the distinct operands by identity, in order of first appearance (x_0 first), and the two slots of every term --
    what the host of multiply_sum derives from pointer equality"""
    distinct, x_slot, y_slot = [], [], []
    for x, y in zip(xs, ys):
        for v, where in ((x, x_slot), (y, y_slot)):
            hit = [i for i, d in enumerate(distinct) if d is v]
            if not hit:
                distinct.append(v)
                hit = [len(distinct) - 1]
            where.append(hit[0])
    return distinct, x_slot, y_slot


def exact_tensor_sum(mods, e, x_slot, y_slot):
    """step 2 of the definition: e [slots][2][count][M][N] any words -> d [3][count][M][N], canonical"""
    d = np.zeros((3,) + e.shape[2:], dtype=object)
    for m, q in enumerate(mods):
        for xs, ys in zip(x_slot, y_slot):
            d[0, :, m] += e[xs, 0, :, m] * e[ys, 0, :, m]
            d[1, :, m] += e[xs, 0, :, m] * e[ys, 1, :, m] + e[xs, 1, :, m] * e[ys, 0, :, m]
            d[2, :, m] += e[xs, 1, :, m] * e[ys, 1, :, m]
        d[:, :, m] %= q
    return d


def extended(cases, L, bits, v, input_ntt):
    """steps 1 to 3 of multiply for one operand [2][count][L][N]: [2][count][M][N] in NTT form over the full base"""
    mods = [c.q for c in cases]
    qs, bs = mods[:L], mods[L:]
    count, n = v.shape[1], v.shape[-1]
    v = np.stack([v[:, :, i, :] % q for i, q in enumerate(qs)], axis=2).reshape(-1, L, n)
    if input_ntt:
        v = transform(cases[:L], v, True)
    return transform(cases, exact_extend(qs, bs, v, bits), False).reshape(2, count, len(mods), n)


def exact_multiply_sum(cases, L, t, bits, xs, ys, input_ntt, output_ntt):
    """the definition: cases = hoisted_exact.host_cases over the full base; xs, ys lists of [2][count][L][N] arrays, the
    same OBJECT where the call passes the same pointer.  Returns (out [3][count][L][N], band [3][count][N])"""
    assert 1 <= len(xs) == len(ys) <= MAX_TERMS
    mods = [c.q for c in cases]
    qs, bs = mods[:L], mods[L:]
    distinct, x_slot, y_slot = slots_of(xs, ys)
    e = np.stack([extended(cases, L, bits, v, input_ntt) for v in distinct])
    count, M, n = e.shape[2:]
    d = exact_tensor_sum(mods, e, x_slot, y_slot)
    stack = transform(cases, d.reshape(-1, M, n), True)
    out = exact_scale_round(qs, bs, t, stack, bits)
    band = in_band(qs, bs, t, stack, bits).reshape(3, count, n)
    if output_ntt:
        out = transform(cases[:L], out, False)
    return out.reshape(3, count, L, n), band


def exact_multiply_relinearize_sum(bfv_cases, ks_cases, L, t, alpha, bits, xs, ys, key, input_ntt, output_ntt):
    """multiply_sum(output_ntt = false), then relinearize(input_ntt = false, output_ntt).  out [2][count][L][N]"""
    m, _ = exact_multiply_sum(bfv_cases, L, t, bits, xs, ys, input_ntt, False)
    return exact_definition(ks_cases, L, alpha, bits, m[:2], m[2], key, False, output_ntt)


def rounding_bound(terms, bands=True):
    """the header's bound on |multiply_sum - sum of `terms` multiply calls| per coefficient, centred: |round(S) - S| <=
    1/2 and |sum_t round(a_t) - S| <= terms / 2 give (terms + 1) / 2 outside the conversion bands; every band hit adds at
    most 1 per rounding, terms + 1 roundings in all"""
    return (terms + 1) / 2 + (terms + 1 if bands else 0)
