"""The arithmetic of KeySwitchPlan.linear_transform_bsgs (include/gpuntt/rns/key_switch.cuh) in Python integers alone, for
tests/test_bsgs_host.py: (a) the word arithmetic of inner_product_galois_giant -- hoist_term's unreduced term with the v
word joined, the exact three-word accumulator across the giant steps, ONE fold -- against the definition's per-step
canonical sums; (b) the ring identity behind "add v_g[0] with multiplier 1": polynomials of Z[X] / (X^N + 1) modulo P Q, a
noiseless switching key, ModDown and the digit decomposition as exact integer maps."""
import math


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
