"""KeySwitchPlan.phase / encrypt_public (include/gpuntt/rns/key_switch.cuh, "Decryption and public-key encryption") and
BfvMultiplyPlan.scale_message / decode (include/gpuntt/rns/bfv_multiply.cuh, "Reading a result back") restated word for
word in Python integers (numpy object arrays: one Python int per word), and true_round: the rounding decode stands for,
with Fraction.  No GPU call and none of the library's arithmetic; the transforms are the in-repo oracle's, as
keygen_exact uses them.  Every step is defined word for word, so what these functions return is compared with
array_equal."""
import math
from fractions import Fraction

import numpy as np

from hoisted_exact import transform
from keygen_exact import exact_lift


def phase_words(qs, ct, s):
    """decrypt_phase: ct [components][count][L][N], s [>= L][N], any words -> (c0 + c1 s + c2 s^2) mod q_m, [count][L][N]"""
    out = np.zeros(ct.shape[1:], dtype=object)
    for m, q in enumerate(qs):
        v = ct[0][:, m, :] + ct[1][:, m, :] * s[m][None, :]
        if ct.shape[0] == 3:
            v = v + ct[2][:, m, :] * (s[m] * s[m])[None, :]
        out[:, m, :] = v % q
    return out


def exact_phase(cases, ct, s, input_ntt, output_ntt):
    """ct [components][count][L][N] (components 2 or 3), s [>= L][N] any words -> out [count][L][N]; cases: the L limbs.
    With input_ntt false ct holds canonical words and is transformed first"""
    ct = np.asarray(ct, dtype=object)
    assert ct.shape[0] in (2, 3) and ct.shape[2] == len(cases)
    if not input_ntt:
        ct = transform(cases, ct, False)
    out = phase_words([c.q for c in cases], ct, s)
    return out if output_ntt else transform(cases, out, True)


def exact_scale_message(qs, t, message):
    """message [count][N] any words -> out [count][L][N] = ((h - r) [t^-1 mod q_i]) mod q_i"""
    Q, h = math.prod(qs), t // 2
    m = np.asarray(message, dtype=object) % t
    r = ((Q % t) * m + h) % t
    out = np.zeros(m.shape[:-1] + (len(qs), m.shape[-1]), dtype=object)
    for i, q in enumerate(qs):
        out[..., i, :] = ((h - r) * pow(t, -1, q)) % q
    return out


def decode_constants(qs, W):
    """qhat_i^-1 mod q_i, R_i = floor(2^(W-1+b_i) / q_i) and b_i, as base_conversion.cuh defines them"""
    Q = math.prod(qs)
    inv = [pow(Q // q, -1, q) if q > 1 else 0 for q in qs]
    blen = [q.bit_length() for q in qs]
    return inv, [(1 << (W - 1 + b)) // q for q, b in zip(qs, blen)], blen


def exact_decode(qs, t, x, W):
    """x [stacks][L][N] any words -> (message [stacks][N], noise words [stacks][N] signed, in_band [stacks][N] bool)"""
    x = np.asarray(x, dtype=object)
    inv, R, blen = decode_constants(qs, W)
    L = len(qs)
    A = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=object)
    Z = np.zeros(A.shape, dtype=object)
    for i, q in enumerate(qs):
        y = (x[..., i, :] * inv[i]) % q
        A = A + (t * y) // q
        Z = Z + ((((t * y) % q) * R[i]) >> (blen[i] - 1))
    S = (A << W) + Z
    half = 1 << (W - 1)
    message = ((S + half) >> W) % t
    noise = ((S + half) % (1 << W)) - half
    low = S % (1 << W)
    in_band = (low >= half - 3 * L) & (low < half)
    return message, noise, in_band.astype(bool)


def noise_max(noise):
    """max_j |n| per stack"""
    return np.array([max(abs(int(v)) for v in row) for row in noise], dtype=object)


def true_round(x, Q, t):
    """round-half-up(t x / Q) mod t and the invariant noise v = t x / Q - round(.), exactly"""
    f = Fraction(t * int(x), Q)
    r = math.floor(f + Fraction(1, 2))
    return r % t, f - r


def combine_public(qs, pk, lifted, message):
    """encrypt_public_combine: pk [2][L][N], lifted [3][count][L][N] = (U, E0, E1), message [count][L][N] or None, any
    words -> out [2][count][L][N]"""
    U, E0, E1 = lifted[0], lifted[1], lifted[2]
    out = np.zeros((2,) + U.shape, dtype=object)
    for m, q in enumerate(qs):
        v = pk[0][m][None, :] * U[:, m, :] + E0[:, m, :]
        if message is not None:
            v = v + message[:, m, :]
        out[0][:, m, :] = v % q
        out[1][:, m, :] = (pk[1][m][None, :] * U[:, m, :] + E1[:, m, :]) % q
    return out


def exact_encrypt_public(cases, pk, small, message):
    """pk [2][L][N] any words, small [3][count][N] signed = (u, e0, e1), message [count][L][N] any words or None ->
    out [2][count][L][N]; cases: the L limbs"""
    return combine_public([c.q for c in cases], pk, exact_lift(cases, small, True), message)
