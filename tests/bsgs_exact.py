"""The arithmetic of KeySwitchPlan.linear_transform_bsgs (include/gpuntt/rns/key_switch.cuh) in Python integers alone:
(a) the word arithmetic of inner_product_galois_giant -- hoist_term's unreduced term with the v word joined, the exact
three-word accumulator across the giant steps, ONE fold -- against the definition's per-step canonical sums; (b) the ring
identity behind "add v_g[0] with multiplier 1": polynomials of Z[X] / (X^N + 1) modulo P Q, a noiseless switching key,
ModDown and the digit decomposition as exact integer maps (both for tests/test_bsgs_host.py); (c) the whole call, steps
1 to 4 of the header's DEFINITION, on numpy object arrays (one Python int per word): no GPU call and none of the
library's arithmetic -- the pieces are those already pinned: hoisted_exact.exact_u, keyswitch_utils.ref_mod_down /
ref_mod_up, the in-repo oracle's transforms, hoisted_exact.finish / rescale_exact.finish_rescale, and pi from
automorphism_index_map (pinned against numpy's sigma by tests/test_galois_host.py).  Every step is defined word for word,
so what (c) returns is compared with array_equal (tests/test_bsgs_exact_host.py, tests/test_gpu_bsgs_exact.py)."""
import math

import numpy as np

from hoisted_exact import exact_u, finish, transform
from keyswitch_utils import ref_mod_down, ref_mod_up
from rescale_exact import finish_rescale


def negacyclic(a, b, mod):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * y
                else:
                    out[k - n] -= x * y
    return [v % mod for v in out]


def sigma(a, k, mod):
    """a(X) -> a(X^k) in Z[X] / (X^N + 1), k odd"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        e = (i * k) % (2 * n)
        out[e % n] += x if e < n else -x
    return [v % mod for v in out]


def centred(x, mod):
    x %= mod
    return x - mod if 2 * x >= mod else x


# ---- (a) the words of the giant kernel ----
def shoup(x, y, q, W):
    """rns_shoup: x any word, y < q with its companion floor(y 2^W / q); returns x y mod q, canonical"""
    yp = (y << W) // q
    r = (x * y - ((x * yp) >> W) * q) & ((1 << W) - 1)
    r = r - q if r >= q else r
    assert r == x * y % q
    return r


class Acc:
    """IpAcc: lo, hi and a carry word; mac is exact for any two words"""

    def __init__(self, W):
        self.W, self.lo, self.hi, self.carry = W, 0, 0, 0

    def mac(self, x, y):
        W, mask = self.W, (1 << self.W) - 1
        assert 0 <= x <= mask and 0 <= y <= mask
        p = x * y
        lo = self.lo + (p & mask)
        hi = self.hi + (p >> W) + (lo >> W)
        self.lo, self.hi, self.carry = lo & mask, hi & mask, self.carry + (hi >> W)

    def value(self):
        return self.lo + (self.hi << self.W) + (self.carry << (2 * self.W))


def fold_sum(acc, q, W):
    """IpFold::sum: three canonical Shoup products, below 3 q < 2^W"""
    t1 = (1 << W) % q
    x = shoup(acc.hi, t1, q, W) + shoup(acc.carry, t1 * t1 % q, q, W) + shoup(acc.lo, 1, q, W)
    assert x < 3 * q < (1 << W) and x % q == acc.value() % q
    return x


def giant_words(digits, keys, v0, plain, q, W):
    """one slot of one modulus, component 0, as inner_product_galois_giant forms it.  digits[g][d], keys[g][d], v0[g]: the
    words of the keyed giant steps (any words); plain: the v words of the steps without a key.  Returns the word"""
    across = Acc(W)
    for dg, kg, vg in zip(digits, keys, v0):
        s = Acc(W)
        for x, k in zip(dg, kg):
            s.mac(x, k)
        x0 = fold_sum(s, q, W)
        x0 = x0 - q if x0 >= q else x0
        x0 += shoup(vg, 1, q, W)  # the v word in c0's place, multiplier 1
        assert x0 < 3 * q < (1 << W)
        across.mac(x0, 1)
    for p in plain:
        across.mac(p, 1)
    assert across.carry <= 64
    x = fold_sum(across, q, W)
    x = x - q if x >= q else x
    return x - q if x >= q else x


def giant_definition(digits, keys, v0, plain, q):
    """the same word through the definition: s_g canonical per giant step, then summed modulo q"""
    t = 0
    for dg, kg, vg in zip(digits, keys, v0):
        s_g = (sum((x % q) * (k % q) for x, k in zip(dg, kg)) + vg % q) % q
        t = (t + s_g) % q
    for p in plain:
        t = (t + p % q) % q
    return t


# ---- (b) the ring identity ----
def giant_step_identity(rng, n, qs, ps, alpha, k, multiplier=1):
    """One keyed giant step on V = (V0, V1) modulo P Q with a noiseless key sigma_k(s) -> s.  Returns (left, right, conv):
    left = s_g[0] + s_g[1] s, right = sigma_k(V0 + V1 s) - sigma_k(conv s), both modulo P Q, and the residue conv that
    ModDown removes.  The two are equal: V0 enters with multiplier 1 because it already lives at scale P (any other
    `multiplier` breaks the identity)."""
    Q, P = math.prod(qs), math.prod(ps)
    PQ = P * Q
    s = [rng.randrange(-1, 2) for _ in range(n)]
    V0 = [rng.randrange(PQ) for _ in range(n)]
    V1 = [rng.randrange(PQ) for _ in range(n)]
    conv = [centred(x, P) for x in V1]
    t = [((x - c) // P) % Q for x, c in zip(V1, conv)]
    assert all((x - c) % P == 0 for x, c in zip(V1, conv))
    parts = [list(range(i, min(i + alpha, len(qs)))) for i in range(0, len(qs), alpha)]
    A = [[0] * n, [0] * n]
    for S in parts:
        Qd = math.prod(qs[i] for i in S)
        gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
        digit = [centred(x, Qd) for x in t]  # any lift of t mod Q_d serves: g_d absorbs the multiple of Q_d
        a_d = [rng.randrange(PQ) for _ in range(n)]
        b_d = [(-x + P * gd * y) % PQ for x, y in zip(negacyclic(a_d, s, PQ), sigma(s, k, PQ))]
        rot = sigma(digit, k, PQ)
        A[0] = [(x + y) % PQ for x, y in zip(A[0], negacyclic(rot, b_d, PQ))]
        A[1] = [(x + y) % PQ for x, y in zip(A[1], negacyclic(rot, a_d, PQ))]
    s0 = [(x + multiplier * y) % PQ for x, y in zip(A[0], sigma(V0, k, PQ))]
    left = [(x + y) % PQ for x, y in zip(s0, negacyclic(A[1], s, PQ))]
    whole = [(x + y) % PQ for x, y in zip(V0, negacyclic(V1, s, PQ))]
    lost = negacyclic([c % PQ for c in conv], s, PQ)
    right = [(x - y) % PQ for x, y in zip(sigma(whole, k, PQ), sigma(lost, k, PQ))]
    return left, right, conv


# ---- (c) the whole call: the header's DEFINITION, steps 1 to 4 ----
# cases: hoisted_exact.host_cases or the MergeCases of a ring (q, logn, poly and the oracle's tables); every array a numpy
# object array of Python integers, ANY word where the header accepts any word.  Keys and weights in the caller's order:
# nothing is reordered here.
def exact_baby(g, cases, L, a, c0, c1, bkeys, belts, key_limbs=None):
    """step 1.  With a key: hoisted_exact.exact_u.  With None: u_b[c][r][m][j] = [m < L] (P mod q_m) (c_c[r][m][j] mod
    q_m) mod q_m, c_0 = c0 (0 if None), c_1 = c1; zero on the special limbs.  a [D][count][M][N], c0 / c1 [count][L][N];
    returns u [n1][2][count][M][N]"""
    c, qs = cases[0], [k.q for k in cases]
    _, count, M, n = a.shape
    P = math.prod(qs[L:])
    u = np.zeros((len(belts), 2, count, M, n), dtype=object)
    for b, key in enumerate(bkeys):
        if key is not None:
            u[b] = exact_u(g, qs, L, c.logn, c.poly, a, c0, [key], [belts[b]], key_limbs)[0]
            continue
        assert c1 is not None, "a baby step without a key needs c1"
        for comp, cc in enumerate((c0, c1)):
            if cc is not None:
                for m, q in enumerate(qs[:L]):
                    u[b, comp, :, m, :] = (P % q) * (cc[:, m, :] % q) % q
    return u


def exact_v(qs, u, row):
    """step 2 for one giant row: v[c][r][m][j] = (sum_{b: row[b] is not None} (row[b][m][j] mod q_m) u_b[c][r][m][j]) mod
    q_m -- None is ABSENT (0), not 1.  row: n1 arrays [M][N] or None; returns [2][count][M][N]"""
    v = np.zeros(u.shape[1:], dtype=object)
    for b, w in enumerate(row):
        if w is None:
            continue
        for m, q in enumerate(qs):
            v[:, :, m, :] = v[:, :, m, :] + u[b, :, :, m, :] * (w[m] % q)[None, None, :]
    for m, q in enumerate(qs):
        v[:, :, m, :] = v[:, :, m, :] % q
    return v


def exact_giant_digits(cases, L, alpha, bits, v1):
    """step 3, the re-decomposition: a' = NTT(mod_up_centred(mod_down(INTT(v_g[1])))).  v1 [stacks][M][N] canonical
    (every stack on its own: the stacks of several giant steps may go through together); returns [D][stacks][M][N]"""
    qs = [k.q for k in cases]
    t = ref_mod_down(qs[:L], qs[L:], transform(cases, v1, True), bits)
    return transform(cases, ref_mod_up(qs[:L], qs[L:], alpha, t, bits, True), False)


def exact_giant(g, cases, digits, v, key, elt, key_limbs=None):
    """step 3, the keyed giant step: s[c][r][m][j] = (sum_d a'[d][r][m][pi(j)] (key[d][c][limb(m)][j] mod q_m)
    + [c = 0] v[0][r][m][pi(j)]) mod q_m for ALL m < M, multiplier 1.  Returns [2][count][M][N]"""
    c, qs = cases[0], [k.q for k in cases]
    D, M = digits.shape[0], len(qs)
    limbs = list(range(M)) if key_limbs is None else list(key_limbs)
    src = g.automorphism_index_map(c.logn, elt, c.poly).astype(np.int64)
    s = np.zeros(v.shape, dtype=object)
    for m, q in enumerate(qs):
        am = (digits[:, :, m, :] % q)[:, :, src]
        for comp in range(2):
            t = (am * (key[:D, comp, limbs[m], :] % q)[:, None, :]).sum(axis=0)
            if comp == 0:
                t = t + (v[0, :, m, :] % q)[:, src]
            s[comp, :, m, :] = t % q
    return s


def exact_bsgs_acc(g, cases, L, alpha, bits, a, c0, c1, bkeys, belts, gkeys, gelts, weights, key_limbs=None):
    """steps 1 to 4 up to the finish: acc[c][r][m][j] = (sum_g s_g[c][r][m][j]) mod q_m, [2][count][M][N] in NTT form"""
    qs = [k.q for k in cases]
    u = exact_baby(g, cases, L, a, c0, c1, bkeys, belts, key_limbs)
    count = u.shape[2]
    v = [exact_v(qs, u, row) for row in weights]
    keyed = [gi for gi, key in enumerate(gkeys) if key is not None]
    if keyed:  # the stacks of every keyed giant step through the transforms and the conversions together: [D][n2k count]
        digits = exact_giant_digits(cases, L, alpha, bits, np.concatenate([v[gi][1] for gi in keyed]))
    acc = np.zeros(u.shape[1:], dtype=object)
    for i, gi in enumerate(keyed):
        v[gi] = exact_giant(g, cases, digits[:, i * count:(i + 1) * count], v[gi], gkeys[gi], gelts[gi], key_limbs)
    for s in v:
        acc = acc + s
    for m, q in enumerate(qs):
        acc[:, :, m, :] = acc[:, :, m, :] % q
    return acc


def exact_linear_transform_bsgs(g, cases, L, alpha, bits, a, c0, c1, bkeys, belts, gkeys, gelts, weights, output_ntt,
                                key_limbs=None, rescale_limbs=0):
    """out [2][count][L][N] ([L - rescale_limbs] with rescale_limbs > 0): the full-base inverse transform, mod_down (or
    mod_down_rescale) and, with output_ntt, the forward transform over the kept moduli"""
    acc = exact_bsgs_acc(g, cases, L, alpha, bits, a, c0, c1, bkeys, belts, gkeys, gelts, weights, key_limbs)
    if rescale_limbs == 0:
        return finish(cases, L, acc, bits, output_ntt)
    M, n = acc.shape[-2:]
    stack = transform(cases, acc.reshape(-1, M, n), True).reshape(acc.shape)
    return finish_rescale(cases, L, rescale_limbs, stack, bits, output_ntt)
