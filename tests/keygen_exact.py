"""KeySwitchPlan.lift_small, generate_keys and encrypt_symmetric (include/gpuntt/rns/key_switch.cuh, "Key material")
restated in Python integers (numpy object arrays: one Python int per word).  THE KEY CONVENTION lives here once for the
tests: key[d] = (-a_d s + e_d + P g_d s_from, a_d) in NTT form over the full base, g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d].
No GPU call and none of the library's arithmetic; the transforms are the in-repo oracle's, as hoisted_exact uses them.
Every step is defined word for word, so what these functions return is compared with array_equal."""
import math

import numpy as np

from hoisted_exact import transform
from keyswitch_utils import crt

EDGES = [-(1 << 31), -1, 0, (1 << 31) - 1]  # the values every lift test plants


def lift(qs, small):
    """small [...][N] signed integers -> [...][len(qs)][N], the canonical residue under every modulus"""
    small = np.asarray(small).astype(object)
    out = np.zeros(small.shape[:-1] + (len(qs), small.shape[-1]), dtype=object)
    for m, q in enumerate(qs):
        out[..., m, :] = small % q  # Python's % of a negative integer is the canonical residue
    return out


def exact_lift(cases, small, to_ntt):
    """lift_small over the moduli of `cases`, with the forward transform when to_ntt"""
    out = lift([c.q for c in cases], small)
    return transform(cases, out, False) if to_ntt else out


def digit_limbs(L, alpha):
    """S_d for every digit: lists of limb indices"""
    alpha = min(alpha, L)
    return [list(range(d * alpha, min((d + 1) * alpha, L))) for d in range(-(-L // alpha))]


def combine_keys(qs, L, alpha, E, s, s_from, a):
    """keygen_combine for keys: E, a [G][D][M][N], s [M][N], s_from [G][M][N], any words -> key0 [G][D][M][N] =
    (E - a s + [m in S_d] (P mod q_m) s_from) mod q_m"""
    P = math.prod(qs[L:])
    out = np.zeros(E.shape, dtype=object)
    assert E.shape[1] == len(digit_limbs(L, alpha))
    for d, S in enumerate(digit_limbs(L, alpha)):
        for m, q in enumerate(qs):
            v = E[:, d, m, :] - a[:, d, m, :] * s[m][None, :]
            if m in S:
                v = v + (P % q) * s_from[:, m, :]
            out[:, d, m, :] = v % q
    return out


def combine_encrypt(qs, L, E, s, message, a):
    """keygen_combine for ciphertexts: E, a [count][L][N], s [>= L][N], message [count][L][N] or None -> c0 [count][L][N]"""
    out = np.zeros(E.shape, dtype=object)
    for m in range(L):
        v = E[:, m, :] - a[:, m, :] * s[m][None, :]
        if message is not None:
            v = v + message[:, m, :]
        out[:, m, :] = v % qs[m]
    return out


def exact_generate_keys(cases, L, alpha, s, s_from, errors, a):
    """s [M][N], s_from [G][M][N], a [G][D][M][N] any words; errors [G][D][N] signed -> key0 [G][D][M][N], with E the
    full-base forward transform of the lifted errors"""
    return combine_keys([c.q for c in cases], L, alpha, exact_lift(cases, errors, True), s, s_from, a)


def exact_encrypt(cases, L, s, errors, message, a):
    """s [>= L][N], errors [count][N] signed, message [count][L][N] or None, a [count][L][N] -> c0 [count][L][N]"""
    return combine_encrypt([c.q for c in cases], L, exact_lift(cases[:L], errors, True), s, message, a)


def gadget(qs, L, alpha):
    """P g_d for every digit, as integers modulo P Q"""
    Q, P = math.prod(qs[:L]), math.prod(qs[L:])
    out = []
    for S in digit_limbs(L, alpha):
        Qd = math.prod(qs[i] for i in S)
        hat = Q // Qd
        out.append(P * hat * pow(hat, -1, Qd))
    return out


def coefficients(cases, x):
    """x [...][len(cases)][N] in NTT form -> the integers modulo the product of the moduli, [...][N]"""
    c = transform(cases, x, True)
    return crt(np.moveaxis(c, -2, 0), [k.q for k in cases])
