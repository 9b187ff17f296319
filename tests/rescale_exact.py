"""The rescaling calls of KeySwitchPlan (include/gpuntt/rns/key_switch.cuh, "Rescaling") restated in Python integers
(numpy object arrays: one Python int per word), on top of relin_exact without changing it.  No GPU call and none of the
library's arithmetic.  The split of the full base into {dropped q, p} -> {kept q} is restated HERE from the header, not
imported from the library: with L' = L - R the input base of mod_down_rescale is limbs L' .. M - 1 of a stack in that
order, the output base limbs 0 .. L' - 1, and the divisor D_R = P q_{L'} ... q_{L-1}; rescale's input base is limbs
L' .. L - 1.  The conversion itself is keyswitch_utils.ref_convert, the restatement of base_conversion.cuh.  Every step is
defined word for word, so what these functions return is compared with array_equal."""
import math

import numpy as np

from hoisted_exact import transform
from keyswitch_utils import ref_convert
from relin_exact import digits_of, inner, tensor


def divide_in_stack(moduli, keep, x, bits):
    """x [stacks][len(moduli)][N], any words: limbs keep .. are the input base, limbs 0 .. keep - 1 the second operand c
    and the output base.  ((c_j - conv_j) D^-1) mod q_j, conv centred, D the product of the input base"""
    kept, dropped = list(moduli[:keep]), list(moduli[keep:])
    D = math.prod(dropped)
    conv = ref_convert(dropped, kept, np.moveaxis(x[:, keep:, :], 1, 0), bits, True)
    out = np.zeros((x.shape[0], keep, x.shape[2]), dtype=object)
    for j, q in enumerate(kept):
        out[:, j, :] = (x[:, j, :] % q - conv[j]) * pow(D, -1, q) % q
    return out


def ref_mod_down_rescale(qs, ps, R, x, bits):
    """x [stacks][M][N] (coefficient form, full base) -> [stacks][L - R][N]"""
    return divide_in_stack(list(qs) + list(ps), len(qs) - R, x, bits)


def ref_rescale(qs, R, x, bits):
    """x [stacks][L][N] (coefficient form, q-base) -> [stacks][L - R][N]"""
    return divide_in_stack(list(qs), len(qs) - R, x, bits)


def in_band(moduli, x, bits):
    """base_conversion.cuh's rounding band, exactly: x [len(moduli)][...] any words, X the integer in [0, Q) with these
    residues; True where X / Q lies in [1/2, 1/2 + eps), eps = 3 len(moduli) / 2^W -- where the centred conversion may
    return the representative above Q / 2 instead of the one below"""
    Q = math.prod(moduli)
    X = 0
    for i, q in enumerate(moduli):
        X = X + (x[i] % q) * ((Q // q) * pow(Q // q, -1, q))
    X = X % Q
    lo = np.asarray(2 * X >= Q, dtype=bool)
    hi = np.asarray(X * (1 << bits) < (Q << (bits - 1)) + 3 * len(moduli) * Q, dtype=bool)
    return lo & hi


def finish_rescale(cases, L, R, stack, bits, output_ntt):
    """stack [...][M][N] in coefficient form -> mod_down_rescale, the forward transform over the kept moduli when
    output_ntt: [...][L - R][N]"""
    M, n = stack.shape[-2:]
    qs = [c.q for c in cases]
    out = ref_mod_down_rescale(qs[:L], qs[L:], R, stack.reshape(-1, M, n), bits)
    if output_ntt:
        out = transform(cases[:L - R], out, False)
    return out.reshape(stack.shape[:-2] + (L - R, n))


def switched_accumulators(cases, L, alpha, bits, d2, key, key_limbs=None):
    """the accumulators of switch_digits for decompose(d2, input_ntt = true): [2][count][M][N], NTT form, canonical"""
    qs = [c.q for c in cases]
    return inner(qs, digits_of(cases, L, alpha, bits, d2), key, key_limbs)


def exact_definition_rescale(cases, L, R, alpha, bits, x, y, key, output_ntt, key_limbs=None):
    """the header's definition of multiply_relinearize_rescale: the accumulators of the key switch of d2 taken to
    coefficient form, P d_c (d_c inverse-transformed over the q-base) added to their q-limbs THERE, then mod_down_rescale
    and the forward transform over the kept moduli.  out [2][count][L - R][N]"""
    qs = [c.q for c in cases]
    P = math.prod(qs[L:])
    d = tensor(qs, L, x, y)
    acc = switched_accumulators(cases, L, alpha, bits, d[2], key, key_limbs)
    M, n = acc.shape[-2:]
    stack = transform(cases, acc.reshape(-1, M, n), True).reshape(acc.shape)
    for c in range(2):
        dc = transform(cases[:L], d[c], True)
        for m, q in enumerate(qs[:L]):
            stack[c, :, m, :] = (stack[c, :, m, :] + P * dc[:, m, :]) % q
    return finish_rescale(cases, L, R, stack, bits, output_ntt)


def folded_stack(cases, L, alpha, bits, x, y, key, key_limbs=None):
    """what runs up to the ModDown: acc[c][r][m][j] = (sum_d a key + [m < L] (P mod q_m) d_c) mod q_m in the NTT domain,
    then the full-base inverse transform.  [2][count][M][N], coefficient form"""
    qs = [c.q for c in cases]
    P = math.prod(qs[L:])
    d = tensor(qs, L, x, y)
    acc = switched_accumulators(cases, L, alpha, bits, d[2], key, key_limbs)
    for m, q in enumerate(qs[:L]):
        acc[:, :, m, :] = (acc[:, :, m, :] + (P % q) * d[:2, :, m, :]) % q
    M, n = acc.shape[-2:]
    return transform(cases, acc.reshape(-1, M, n), True).reshape(acc.shape)


def exact_multiply_relinearize_rescale(cases, L, R, alpha, bits, x, y, key, output_ntt, key_limbs=None):
    """the folded form with mod_down_rescale as its ModDown.  out [2][count][L - R][N]"""
    return finish_rescale(cases, L, R, folded_stack(cases, L, alpha, bits, x, y, key, key_limbs), bits, output_ntt)


def centred_difference(kept, a, b):
    """a, b [...][len(kept)][N] canonical: the integers they are the residues of, subtracted and centred modulo the
    product of the kept base.  [...][N]"""
    Q = math.prod(kept)
    s = 0
    for j, q in enumerate(kept):
        s = s + ((a[..., j, :] - b[..., j, :]) % q) * ((Q // q) * pow(Q // q, -1, q))
    return (s + Q // 2) % Q - Q // 2
