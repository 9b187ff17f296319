"""The samplers of include/gpuntt/rns/sampling.cuh restated in Python integers: Philox4x32-10, the bounded rejection of
sample_uniform (k candidates per block, 32 candidates, then the last r mod q) and the two small distributions.  No GPU
call and none of the library's code; what these functions return is compared word for word."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
TERNARY, CBD21 = 0, 1
MAX_CANDIDATES = 32


def philox(ctr, key):
    """Philox4x32-10 (Random123): ctr 4 words, key 2 words -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [c0, c1, c2, c3]


def candidates(w, bits, seed, stream_id, count):
    """the first `count` candidates of word w"""
    k = 2 if bits == 64 else 4
    key = (seed & MASK32, (seed >> 32) & MASK32)
    out = []
    for c in range(count):
        if c % k == 0:
            b = philox((w & MASK32, (w >> 32) & MASK32, c // k, stream_id), key)
        out.append(b[2 * (c % 2)] | b[2 * (c % 2) + 1] << 32 if bits == 64 else b[c % 4])
    return out


def uniform_word(w, q, bits, seed, stream_id, max_candidates=MAX_CANDIDATES):
    """(the word, the candidates it looked at)"""
    mask = (1 << q.bit_length()) - 1
    r = 0
    for used, cand in enumerate(candidates(w, bits, seed, stream_id, max_candidates)):
        r = cand & mask
        if r < q:
            return r, used + 1
    return r % q, max_candidates


def exact_uniform(moduli, n_power, stacks, bits, seed, stream_id, max_candidates=MAX_CANDIDATES):
    """([stacks][len(moduli)][N] object words, the same shape of candidate counts)"""
    n, K = 1 << n_power, len(moduli)
    out = np.zeros((stacks, K, n), dtype=object)
    used = np.zeros((stacks, K, n), dtype=np.int64)
    for s in range(stacks):
        for m, q in enumerate(moduli):
            for j in range(n):
                out[s, m, j], used[s, m, j] = uniform_word((s * K + m) * n + j, int(q), bits, seed, stream_id,
                                                           max_candidates)
    return out, used


def small_word(w, distribution, seed, stream_id):
    b = philox((w & MASK32, (w >> 32) & MASK32, 0, stream_id), (seed & MASK32, (seed >> 32) & MASK32))
    if distribution == CBD21:
        x = b[0] | b[1] << 32
        m21 = (1 << 21) - 1
        return bin(x & m21).count("1") - bin((x >> 21) & m21).count("1")
    x = b[0] | b[1] << 32 | b[2] << 64 | b[3] << 96
    for f in range(64):
        v = (x >> (2 * f)) & 3
        if v != 3:
            return v - 1
    return 0


def exact_small(polys, n_power, distribution, seed, stream_id):
    """int32 [polys][N]"""
    n = 1 << n_power
    return np.array([small_word(w, distribution, seed, stream_id) for w in range(polys * n)],
                    dtype=np.int32).reshape(polys, n)
