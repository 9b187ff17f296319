"""BfvMultiplyPlan (include/gpuntt/rns/bfv_multiply.cuh) restated in Python integers (numpy object arrays: one Python int
per word, as keyswitch_utils does).  No GPU call and none of the library's arithmetic: the conversions are
keyswitch_utils.ref_convert (the formulas of base_conversion.cuh), the transforms the in-repo oracle's restated NTTCPU
(hoisted_exact.transform over hoisted_exact.host_cases).  Every step is defined word for word, so what these functions
return is compared with array_equal.  Beside the definition: the exact rounding band of scale_round's first conversion
and the ideal value round(t D / Q) the definition stands for."""
import math

import numpy as np

from hoisted_exact import transform
from keyswitch_utils import centre, crt, negacyclic, ref_convert


def exact_extend(qs, bs, x, bits):
    """x [stacks][L][N] any words -> full [stacks][M][N]: the q-limbs reduced, the b-limbs the centred conversion"""
    L = len(qs)
    full = np.zeros((x.shape[0], L + len(bs), x.shape[2]), dtype=object)
    for i, q in enumerate(qs):
        full[:, i, :] = x[:, i, :] % q
    conv = ref_convert(list(qs), list(bs), np.moveaxis(x, 1, 0), bits, True)
    for j in range(len(bs)):
        full[:, L + j, :] = conv[j]
    return full


def scaled(qs, bs, t, full):
    """step 1 of scale_round: s_m = ((t mod m_m) full_m) mod m_m, [M][stacks][N]"""
    return np.stack([(t % m) * (full[:, i, :] % m) % m for i, m in enumerate(list(qs) + list(bs))])


def exact_scale_round(qs, bs, t, full, bits):
    """full [stacks][M][N] any words -> out [stacks][L][N], the three steps of the header"""
    L, Q = len(qs), math.prod(qs)
    s = scaled(qs, bs, t, full)
    conv = ref_convert(list(qs), list(bs), s[:L], bits, True)
    r = np.stack([(s[L + j] - conv[j]) * pow(Q, -1, b) % b for j, b in enumerate(bs)])
    return np.moveaxis(ref_convert(list(bs), list(qs), r, bits, True), 0, 1)


def in_band(qs, bs, t, full, bits):
    """[stacks][N] booleans: the q-limbs of t X lie in the rounding band [1/2, 1/2 + eps) Q of step 2's conversion, eps =
    3 L / 2^W (base_conversion.cuh) -- the only place where scale_round may differ from round(t X / Q), by one"""
    L, Q = len(qs), math.prod(qs)
    xt = crt(scaled(qs, bs, t, full)[:L], list(qs))
    return np.array(2 * xt >= Q, dtype=bool) & np.array(xt * (1 << bits) < Q * ((1 << (bits - 1)) + 3 * L), dtype=bool)


def ideal(t, D, Q):
    """round(t D / Q), halves up, for an object array of integers D"""
    return (2 * t * D + Q) // (2 * Q)


def representatives(qs, bs, full):
    """the integers extend chose: full [stacks][M][N] (what exact_extend returns) -> the value in (-QB/2, QB/2) with
    those residues, [stacks][N]; extend's choice has magnitude at most Q (1/2 + eps) and B > Q, so it is this one"""
    mods = list(qs) + list(bs)
    return centre(crt(np.moveaxis(full, 1, 0), mods), math.prod(mods))


def integer_tensor(x_rep, y_rep):
    """x_rep, y_rep [2][count][N] integers -> D [3][count][N] = (x0 y0, x0 y1 + x1 y0, x1 y1) in Z[X] / (X^N + 1)"""
    count = x_rep.shape[1]
    D = np.zeros((3,) + x_rep.shape[1:], dtype=object)
    for r in range(count):
        D[0, r] = negacyclic(x_rep[0, r], y_rep[0, r])
        D[1, r] = negacyclic(x_rep[0, r], y_rep[1, r]) + negacyclic(x_rep[1, r], y_rep[0, r])
        D[2, r] = negacyclic(x_rep[1, r], y_rep[1, r])
    return D


def exact_multiply(cases, L, t, bits, x, y, input_ntt, output_ntt):
    """the seven steps of multiply: cases = hoisted_exact.host_cases over the full base; x, y [2][count][L][N] any words
    (read modulo q_m); returns (out [3][count][L][N], band [3][count][N])"""
    mods = [c.q for c in cases]
    qs, bs = mods[:L], mods[L:]
    M, n, count = len(mods), x.shape[-1], x.shape[1]
    full = []
    for v in (x, y):
        v = np.stack([v[:, :, i, :] % q for i, q in enumerate(qs)], axis=2).reshape(-1, L, n)
        if input_ntt:
            v = transform(cases[:L], v, True)
        full.append(transform(cases, exact_extend(qs, bs, v, bits), False).reshape(2, count, M, n))
    xe, ye = full
    d = np.zeros((3, count, M, n), dtype=object)
    for m, q in enumerate(mods):
        d[0, :, m] = xe[0, :, m] * ye[0, :, m] % q
        d[1, :, m] = (xe[0, :, m] * ye[1, :, m] + xe[1, :, m] * ye[0, :, m]) % q
        d[2, :, m] = xe[1, :, m] * ye[1, :, m] % q
    stack = transform(cases, d.reshape(-1, M, n), True)
    out = exact_scale_round(qs, bs, t, stack, bits)
    band = in_band(qs, bs, t, stack, bits).reshape(3, count, n)
    if output_ntt:
        out = transform(cases[:L], out, False)
    return out.reshape(3, count, L, n), band
