"""KeySwitchPlan.mod_down_add, KeySwitchPlan.relinearize (include/gpuntt/rns/key_switch.cuh) and
BfvMultiplyPlan.multiply_relinearize (include/gpuntt/rns/bfv_multiply.cuh) restated in Python integers (numpy object
arrays: one Python int per word).  relinearize twice: the DEFINITION of the header (apply on c2, then c01 added modulo
q_m in the output's form) and what RUNS (P c01 joined to the accumulators before the ModDown in NTT form; c01 added in
mod_down's epilogue in coefficient form).  No GPU call and none of the library's arithmetic: relin_exact, hoisted_exact,
bfv_exact and keyswitch_utils are imported, not edited.  Every step is defined word for word, so what these functions
return is compared with array_equal."""
import math

import numpy as np

from bfv_exact import exact_multiply
from hoisted_exact import finish, transform
from keyswitch_utils import ref_mod_down, ref_mod_up
from relin_exact import digits_of, inner


def reduce_limbs(qs, x):
    """x [...][len(qs)][N] any words -> the same words modulo their limb's modulus"""
    out = np.zeros(x.shape, dtype=object)
    for m, q in enumerate(qs):
        out[..., m, :] = x[..., m, :] % q
    return out


def exact_mod_down_add(qs, ps, x, addend, bits):
    """x [stacks][M][N], addend [stacks][L][N] any words -> (mod_down(x) + (addend mod q_j)) mod q_j, [stacks][L][N]"""
    out = ref_mod_down(list(qs), list(ps), x, bits)
    for j, q in enumerate(qs):
        out[:, j, :] = (out[:, j, :] + addend[:, j, :] % q) % q
    return out


def exact_seeded(qs, L, a, key, c01, key_limbs=None):
    """inner_product_seeded: acc[c][r][m][j] = (sum_d a key + [m < L] (P mod q_m) c01[c][r][m][j]) mod q_m.
    a [D][count][M][N], c01 [2][count][L][N] any words -> [2][count][M][N]"""
    P = math.prod(qs[L:])
    acc = inner(qs, a, key, key_limbs)
    for m, q in enumerate(qs[:L]):
        acc[:, :, m, :] = (acc[:, :, m, :] + (P % q) * c01[:, :, m, :]) % q
    return acc


def digits(cases, L, alpha, bits, c2, input_ntt):
    """the plan's decompose on c2 [count][L][N]: residues in NTT form, any word in coefficient form"""
    qs = [c.q for c in cases]
    if input_ntt:
        return digits_of(cases, L, alpha, bits, c2)
    return transform(cases, ref_mod_up(qs[:L], qs[L:], alpha, c2, bits, True), False)


def exact_definition(cases, L, alpha, bits, c01, c2, key, input_ntt, output_ntt, key_limbs=None):
    """the header: k = apply(c2); out[c] = (k[c] + c01[c]) mod q_m, c01 reduced and brought to the output's form by the
    q-base transform when input_ntt != output_ntt.  out [2][count][L][N]"""
    qs = [c.q for c in cases]
    k = finish(cases, L, inner(qs, digits(cases, L, alpha, bits, c2, input_ntt), key, key_limbs), bits, output_ntt)
    low = reduce_limbs(qs[:L], c01)
    if input_ntt != output_ntt:
        low = transform(cases[:L], low.reshape((-1,) + low.shape[-2:]), input_ntt).reshape(low.shape)
    return reduce_limbs(qs[:L], k + low)


def exact_relinearize(cases, L, alpha, bits, c01, c2, key, input_ntt, output_ntt, key_limbs=None):
    """what runs: inner_product_seeded and finish (input_ntt), or the plain inner product, the full-base inverse
    transform, mod_down_add and the optional q-base transform.  out [2][count][L][N]"""
    qs = [c.q for c in cases]
    a = digits(cases, L, alpha, bits, c2, input_ntt)
    if input_ntt:
        return finish(cases, L, exact_seeded(qs, L, a, key, c01, key_limbs), bits, output_ntt)
    acc = inner(qs, a, key, key_limbs)
    M, n = acc.shape[-2:]
    stack = transform(cases, acc.reshape(-1, M, n), True)
    out = exact_mod_down_add(qs[:L], qs[L:], stack, c01.reshape(-1, L, n), bits)
    if output_ntt:
        out = transform(cases[:L], out, False)
    return out.reshape(c01.shape)


def exact_bfv_multiply_relinearize(bfv_cases, ks_cases, L, t, alpha, bits, x, y, key, input_ntt, output_ntt):
    """multiply(output_ntt = false), then relinearize(input_ntt = false, output_ntt); bfv_cases over {q, b}, ks_cases
    over {q, p}.  out [2][count][L][N]"""
    m, _ = exact_multiply(bfv_cases, L, t, bits, x, y, input_ntt, False)
    return exact_definition(ks_cases, L, alpha, bits, m[:2], m[2], key, False, output_ntt)
