"""KeySwitchPlan.multiply_relinearize (include/gpuntt/rns/key_switch.cuh) restated in Python integers (numpy object
arrays: one Python int per word), twice: the three-step DEFINITION of the header (the tensor terms, apply on d2, the two
additions after the ModDown) and the FOLDED form the kernels compute (P d_c joined to the accumulators before the
ModDown).  No GPU call and none of the library's arithmetic: the transforms are the in-repo oracle's restated NTTCPU
(hoisted_exact.transform), the ModUp and ModDown are keyswitch_utils' restatements of base_conversion.cuh.  Every step is
defined word for word, so what these functions return is compared with array_equal."""
import math

import numpy as np

from hoisted_exact import finish, transform
from keyswitch_utils import ref_mod_up


def tensor(qs, L, x, y):
    """x, y [2][count][L][N], any words, read modulo q_m -> d [3][count][L][N]: d0 = x0 y0, d1 = x0 y1 + x1 y0,
    d2 = x1 y1, canonical"""
    d = np.zeros((3,) + x.shape[1:], dtype=object)
    for m, q in enumerate(qs[:L]):
        x0, x1, y0, y1 = x[0, :, m] % q, x[1, :, m] % q, y[0, :, m] % q, y[1, :, m] % q
        d[0, :, m], d[1, :, m], d[2, :, m] = x0 * y0 % q, (x0 * y1 + x1 * y0) % q, x1 * y1 % q
    return d


def digits_of(cases, L, alpha, bits, d2):
    """decompose(d2, input_ntt = true): the q-base inverse transform, the centred ModUp, the full-base forward transform.
    d2 [count][L][N] canonical -> a [D][count][M][N]"""
    qs = [c.q for c in cases]
    coeff = transform(cases[:L], d2, True)
    return transform(cases, ref_mod_up(qs[:L], qs[L:], alpha, coeff, bits, True), False)


def inner(qs, a, key, key_limbs=None):
    """acc[c][r][m][j] = (sum_d a[d][r][m][j] key[d][c][limb(m)][j]) mod q_m, the key read modulo q_m.
    a [D][count][M][N], key [D_key][2][key_mod_count][N] -> [2][count][M][N]"""
    D, count, M, n = a.shape
    limbs = list(range(M)) if key_limbs is None else list(key_limbs)
    acc = np.zeros((2, count, M, n), dtype=object)
    for m, q in enumerate(qs):
        for c in range(2):
            km = key[:D, c, limbs[m], :] % q
            acc[c, :, m, :] = (a[:, :, m, :] * km[:, None, :]).sum(axis=0) % q
    return acc


def exact_definition(cases, L, alpha, bits, x, y, key, output_ntt, key_limbs=None):
    """the header's three steps: out[c] = (apply(d2)[c] + d_c) mod q_m, d_c inverse-transformed first when output_ntt is
    false.  out [2][count][L][N]"""
    qs = [c.q for c in cases]
    d = tensor(qs, L, x, y)
    k = finish(cases, L, inner(qs, digits_of(cases, L, alpha, bits, d[2]), key, key_limbs), bits, output_ntt)
    out = np.zeros_like(k)
    for c in range(2):
        dc = d[c] if output_ntt else transform(cases[:L], d[c], True)
        for m, q in enumerate(qs[:L]):
            out[c, :, m] = (k[c, :, m] + dc[:, m]) % q
    return out


def exact_multiply_relinearize(cases, L, alpha, bits, x, y, key, output_ntt, key_limbs=None):
    """what runs: acc[c][r][m][j] = (sum_d a key + [m < L] (P mod q_m) d_c) mod q_m, then the plan's own finish.
    out [2][count][L][N]"""
    qs = [c.q for c in cases]
    P = math.prod(qs[L:])
    d = tensor(qs, L, x, y)
    acc = inner(qs, digits_of(cases, L, alpha, bits, d[2]), key, key_limbs)
    for m, q in enumerate(qs[:L]):
        acc[:, :, m, :] = (acc[:, :, m, :] + (P % q) * d[:2, :, m, :]) % q
    return finish(cases, L, acc, bits, output_ntt)
