"""BFV batching (include/gpuntt/rns/bfv_encode.cuh) and the plaintext operands of KeySwitchPlan (lift_centred,
multiply_plain; include/gpuntt/rns/key_switch.cuh, "Plaintext operands") restated in Python integers.  THE SLOT
CONVENTION lives here once for the tests: slot (r, c) of the 2 x N/2 matrix, linear index r N/2 + c, holds a(psi^e) with
e(0, c) = 5^c mod 2N and e(1, c) = 2N - 5^c mod 2N; GPU_NTT writes a(psi^(2 brev(i) + 1)) at place i, so the slot stands
at pos = brev((e - 1) / 2).  No GPU call and none of the library's arithmetic: the transforms are the in-repo oracle's,
as hoisted_exact uses them, and the semantic facts are checked against Horner evaluation and a coefficient-domain sigma_k
written out here.  Everything is defined word for word, so what these functions return is compared with array_equal."""
from types import SimpleNamespace

import numpy as np

from hoisted_exact import transform
from oracle import oracle as O


def brev(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2)


def slot_exponent(slot, n_power):
    """e(r, c) of the linear slot index r N/2 + c"""
    n = 1 << n_power
    r, c = divmod(slot, n // 2)
    e = pow(5, c, 2 * n)
    return e if r == 0 else 2 * n - e


def slot_position(slot, n_power):
    return brev((slot_exponent(slot, n_power) - 1) // 2, n_power)


def slot_maps(n_power):
    """(to_position indexed by slot, to_slot its inverse), as uint32 arrays"""
    n = 1 << n_power
    to_position = np.array([slot_position(s, n_power) for s in range(n)], dtype=np.uint32)
    to_slot = np.zeros(n, dtype=np.uint32)
    to_slot[to_position] = np.arange(n, dtype=np.uint32)
    return to_position, to_slot


def psi_of(t, n_power):
    """a primitive 2N-th root of unity modulo the prime t = 1 mod 2N"""
    n = 1 << n_power
    assert (t - 1) % (2 * n) == 0
    b = 2
    while True:
        psi = pow(b, (t - 1) // (2 * n), t)
        if pow(psi, n, t) == t - 1:
            return psi
        b += 1


def plain_factors(t, n_power):
    """(t, omega, psi): what NTTParameters and the oracle take as `factors`"""
    psi = psi_of(t, n_power)
    return t, psi * psi % t, psi


def plain_case(bits, n_power, t):
    """the oracle's tables modulo t: what hoisted_exact.transform reads of a case"""
    P = O.Port(bits)
    return SimpleNamespace(P=P, logn=n_power, n=1 << n_power, poly=O.X_N_plus, q=t,
                           oprm=P.merge_params(n_power, O.X_N_plus, plain_factors(t, n_power)))


def exact_encode(case, values):
    """values [count][N] any words by slot -> the coefficients modulo t, [count][N]: w[pos(slot)] = value mod t, then the
    inverse transform"""
    to_position, _ = slot_maps(case.logn)
    w = np.zeros(values.shape, dtype=object)
    w[:, to_position.astype(np.int64)] = values % case.q
    return transform([case], w[:, None, :], True)[:, 0, :]


def exact_decode(case, plain):
    """plain [count][N] canonical coefficients -> the slot values [count][N]"""
    to_position, _ = slot_maps(case.logn)
    return transform([case], plain[:, None, :], False)[:, 0, :][:, to_position.astype(np.int64)]


def horner_slots(plain, t, psi, n_power):
    """a(psi^e(slot)) for every slot, by Horner's rule: nothing of the transforms"""
    out = []
    for slot in range(1 << n_power):
        x, acc = pow(psi, slot_exponent(slot, n_power), t), 0
        for coeff in reversed([int(v) for v in plain]):
            acc = (acc * x + coeff) % t
        out.append(acc)
    return np.array(out, dtype=object)


def sigma(plain, k, t):
    """a(X) -> a(X^k) in Z_t[X]/(X^N + 1), coefficient by coefficient"""
    n = len(plain)
    out = np.zeros(n, dtype=object)
    for j, v in enumerate(plain):
        e = (j * k) % (2 * n)
        out[e % n] = (out[e % n] + (int(v) if e < n else -int(v))) % t
    return out


def negacyclic_product(a, b, t):
    n = len(a)
    out = np.zeros(n, dtype=object)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            s = int(x) * int(y)
            out[(i + j) % n] = (out[(i + j) % n] + (s if i + j < n else -s)) % t
    return out


def rotate_rows(values, s):
    """both rows of [...][N] slot values rotated LEFT by s: new[r][c] = old[r][(c + s) mod N/2]"""
    half = values.shape[-1] // 2
    rows = values.reshape(values.shape[:-1] + (2, half))
    return np.roll(rows, -s, axis=-1).reshape(values.shape)


def swap_rows(values):
    half = values.shape[-1] // 2
    return np.concatenate([values[..., half:], values[..., :half]], axis=-1)


def centre(words, t):
    """m = word mod t; m - t from (t + 1) >> 1 on"""
    m = words % t
    return np.where(m >= (t + 1) >> 1, m - t, m)


def lift_centred(qs, t, words):
    """words [...][N] any words -> [...][len(qs)][N], the canonical residue of the centred value under every modulus"""
    v = centre(np.asarray(words).astype(object), t)
    out = np.zeros(v.shape[:-1] + (len(qs), v.shape[-1]), dtype=object)
    for i, q in enumerate(qs):
        out[..., i, :] = v % q  # Python's % of a negative integer is the canonical residue
    return out


def exact_lift_centred(cases, t, words, to_ntt):
    """KeySwitchPlan.lift_centred over the moduli of `cases`, with the forward transform when to_ntt"""
    out = lift_centred([c.q for c in cases], t, words)
    return transform(cases, out, False) if to_ntt else out


def exact_multiply_plain(qs, ct, pt):
    """ct [2][count][L][N], pt [1 or count][L][N], any words -> (ct * pt) mod q_i, [2][count][L][N]"""
    out = np.zeros(ct.shape, dtype=object)
    for i, q in enumerate(qs):
        out[:, :, i, :] = (ct[:, :, i, :] * pt[None, :, i, :]) % q
    return out
