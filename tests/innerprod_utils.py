"""Shared by the RNS inner product tests (include/gpuntt/rns/inner_product.cuh): moduli of mixed widths, random words
with planted extremes and the definition restated in Python integers (numpy object arrays: one Python int per word)."""
import math

import numpy as np

from gpu_utils import find_ntt_factors

WIDTHS = {64: (62, 61, 60, 45, 20), 32: (30, 29, 20)}
COMPOSITES = {64: (15015, 215441, 47027 * 43, (2 ** 31 - 1) * (2 ** 29 - 3)), 32: (15015, 215441, 47027 * 43)}

_pools = {}


def moduli(bits, need):
    """`need` moduli of mixed widths: NTT primes found by search (every width of WIDTHS within the first few), a few
    odd composites in between"""
    pool, used = _pools.setdefault(bits, ([], {}))
    while len(pool) < need:
        i = len(pool)
        if i % 6 == 3 and i // 6 < len(COMPOSITES[bits]):
            m = COMPOSITES[bits][i // 6]
        else:
            w = WIDTHS[bits][(i - (i + 2) // 6) % len(WIDTHS[bits])]
            m = find_ntt_factors(w, 3, skip=used.get(w, 0), clear_of_top=True)[0]
            used[w] = used.get(w, 0) + 1
        assert all(math.gcd(m, o) == 1 for o in pool), m
        pool.append(m)
    return pool[:need]


def random_words(rng, shape, bits, plant=()):
    """uniform words of the whole range as an object array; `plant`: values written at a few scattered places"""
    hi = 1 << bits
    x = rng.integers(0, hi, size=shape, dtype=np.uint64, endpoint=False) if bits == 64 else \
        rng.integers(0, hi, size=shape, dtype=np.uint64)
    x = x.astype(object)
    flat = x.reshape(-1)
    for i, v in enumerate(plant):
        flat[(7 * i + 3 * (i // 2)) % flat.size] = v
        flat[flat.size - 1 - (5 * i) % flat.size] = v
    return x


def operands(rng, bits, qs, n_power, D, C, count, key_digits, key_mod_count):
    """a [D][count][M][N], key [key_digits][C][key_mod_count][N], out0 [C][count][M][N]: any word value, with 0,
    q - 1 for every modulus and 2^W - 1 planted"""
    M, n, top = len(qs), 1 << n_power, (1 << bits) - 1
    plant = [0, top] + [q - 1 for q in qs] + [top, 0]
    a = random_words(rng, (D, count, M, n), bits, plant)
    key = random_words(rng, (key_digits, C, key_mod_count, n), bits, plant[::-1])
    out0 = random_words(rng, (C, count, M, n), bits, plant)
    # one place where every factor and the prefilled word are extreme at once
    a[:, 0, M - 1, n - 1] = top
    key[:, :, :, n - 1] = top
    out0[:, 0, M - 1, n - 1] = top
    return a, key, out0


def ref_inner_product(qs, a, key, out0, D, limbs=None, accumulate=False):
    """the definition, in Python integers: returns out [C][count][M][N]"""
    M = len(qs)
    C = key.shape[1]
    limbs = list(range(M)) if limbs is None else limbs
    out = np.zeros((C,) + a.shape[1:], dtype=object)
    for c in range(C):
        for m, q in enumerate(qs):
            s = out0[c, :, m, :] if accumulate else 0
            for d in range(D):
                s = s + a[d, :, m, :] * key[d, c, limbs[m], :][None, :]
            out[c, :, m, :] = s % q
    return out


def words(g, x, bits):
    """object array -> flat numpy array of the word type"""
    return np.ascontiguousarray(x.astype(np.uint64).astype(g.np_dtype(bits)).reshape(-1))


def from_words(x, shape):
    return np.asarray(x).astype(np.uint64).astype(object).reshape(shape)
