"""KeySwitchPlan.multiply_relinearize_sum (include/gpuntt/rns/key_switch.cuh) restated in Python integers (numpy object
arrays: one Python int per word), twice: the three-step DEFINITION of the header (the tensor terms summed over the pairs,
apply on d2, the two additions after the ModDown) and the FOLDED form the kernels compute (P d_c joined to the
accumulators before the ModDown).  No GPU call and none of the library's arithmetic: everything but the sum over the
terms is relin_exact's (digits_of, inner, finish)."""
import math

import numpy as np

from hoisted_exact import finish, transform
from relin_exact import digits_of, inner


def tensor_sum(qs, L, xs, ys):
    """xs, ys: lists of T arrays [2][count][L][N], any words, read modulo q_m -> d [3][count][L][N]:
    d0 = sum_t x0 y0, d1 = sum_t x0 y1 + x1 y0, d2 = sum_t x1 y1, canonical"""
    assert len(xs) == len(ys) and xs
    d = np.zeros((3,) + xs[0].shape[1:], dtype=object)
    for m, q in enumerate(qs[:L]):
        for x, y in zip(xs, ys):
            x0, x1, y0, y1 = x[0, :, m] % q, x[1, :, m] % q, y[0, :, m] % q, y[1, :, m] % q
            d[0, :, m] += x0 * y0
            d[1, :, m] += x0 * y1 + x1 * y0
            d[2, :, m] += x1 * y1
        d[:, :, m] %= q
    return d


def exact_sum_definition(cases, L, alpha, bits, xs, ys, key, output_ntt, key_limbs=None):
    """the header's three steps: out[c] = (apply(d2)[c] + d_c) mod q_m, d_c inverse-transformed first when output_ntt is
    false.  out [2][count][L][N]"""
    qs = [c.q for c in cases]
    d = tensor_sum(qs, L, xs, ys)
    k = finish(cases, L, inner(qs, digits_of(cases, L, alpha, bits, d[2]), key, key_limbs), bits, output_ntt)
    out = np.zeros_like(k)
    for c in range(2):
        dc = d[c] if output_ntt else transform(cases[:L], d[c], True)
        for m, q in enumerate(qs[:L]):
            out[c, :, m] = (k[c, :, m] + dc[:, m]) % q
    return out


def exact_multiply_relinearize_sum(cases, L, alpha, bits, xs, ys, key, output_ntt, key_limbs=None):
    """what runs: acc[c][r][m][j] = (sum_d a key + [m < L] (P mod q_m) d_c) mod q_m, then the plan's own finish.
    out [2][count][L][N]"""
    qs = [c.q for c in cases]
    P = math.prod(qs[L:])
    d = tensor_sum(qs, L, xs, ys)
    acc = inner(qs, digits_of(cases, L, alpha, bits, d[2]), key, key_limbs)
    for m, q in enumerate(qs[:L]):
        acc[:, :, m, :] = (acc[:, :, m, :] + (P % q) * d[:2, :, m, :]) % q
    return finish(cases, L, acc, bits, output_ntt)
