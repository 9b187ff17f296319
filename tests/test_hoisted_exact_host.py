"""The exact-integer reference of rotate_hoisted / rotate_hoisted_sum (tests/hoisted_exact.py) checked on its own, no
GPU: on a noiseless instance its output decrypts to sigma_k(m) and to sum_g pt_g sigma_k(m) within the bounds the GPU
tests derive, on rings of 62/61-bit and of 30/29-bit primes; and for one identity element without c0 and weights its
accumulator is the exact inner product of innerprod_utils."""
import math
import os

import numpy as np
import pytest

from hoisted_exact import WIDE, exact_rotate_hoisted, exact_rotate_hoisted_sum, exact_u, host_cases, transform
from innerprod_utils import operands, ref_inner_product
from keyswitch_utils import centre, crt, negacyclic, partition, ref_mod_up


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def sigma(x, k):
    """a(X) -> a(X^k) in Z[X] / (X^N + 1)"""
    n = len(x)
    out = np.zeros(n, dtype=object)
    for i in range(n):
        e = (i * k) % (2 * n)
        out[e % n] += x[i] if e < n else -x[i]
    return out


def noiseless_instance(g, bits, rng):
    """test_gpu_hoisted_rotation.test_it_really_rotates' instance with every step in Python integers and the oracle's
    transforms: c0 + c1 s = msg (mod Q); for k = rotation by 1 and conjugation the key
    key_k[d] = (-a_d s + P g_d sigma_k(s), a_d), g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d]; weights pt_g small signed
    polynomials; a = the centred ModUp of c1, transformed"""
    n_power, L, K, alpha = 5, 3, 2, 2
    M, n = L + K, 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], M)
    full = [c.q for c in cases]
    assert [q.bit_length() for q in full] == [WIDE[bits][i % 4] for i in range(M)]
    qs, ps = full[:L], full[L:]
    Q, P = math.prod(qs), math.prod(ps)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    elts = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_conjugation(n_power)]
    parts = partition(L, alpha)
    keys, weights, pts = [], [], []
    for k in elts:
        key = np.zeros((len(parts), 2, M, n), dtype=object)
        for d, S in enumerate(parts):
            Qd = math.prod(qs[i] for i in S)
            gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
            a_d = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(n)], dtype=object)
            b_d = -negacyclic(a_d, s) + P * gd * sigma(s, k)
            for m, q in enumerate(full):
                key[d, 0, m], key[d, 1, m] = b_d % q, a_d % q
        keys.append(transform(cases, key, False))
        pt = np.array([int(v) for v in rng.integers(-50, 51, size=n)], dtype=object)
        weights.append(transform(cases, np.array([pt % q for q in full], dtype=object), False))
        pts.append(pt)
    c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
    msg = np.array([int(v) for v in rng.integers(-1000, 1000, size=n)], dtype=object)
    c0 = (msg - negacyclic(c1, s)) % Q
    a = transform(cases, ref_mod_up(qs, ps, alpha, np.array([[c1 % q for q in qs]], dtype=object), bits, True), False)
    c0 = transform(cases[:L], np.array([[c0 % q for q in qs]], dtype=object), False)
    return SimpleInstance(cases=cases, L=L, qs=qs, Q=Q, s=s, elts=elts, keys=keys, weights=weights, pts=pts, msg=msg,
                          a=a, c0=c0)


class SimpleInstance:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_reference_really_rotates(g, bits):
    """out_0 + out_1 s - sigma_k(msg), centred mod Q, within (1 + h) / 2 + 1, h = |s|_1: the bound
    test_it_really_rotates states"""
    t = noiseless_instance(g, bits, np.random.default_rng(23 + bits))
    bound = (1 + int(sum(abs(v) for v in t.s))) / 2 + 1
    for output_ntt in (False, True):
        out = exact_rotate_hoisted(g, t.cases, t.L, bits, t.a, t.c0, t.keys, t.elts, output_ntt)
        if output_ntt:
            out = transform(t.cases[:t.L], out, True)
        for i, k in enumerate(t.elts):
            value = crt(out[i, 0, 0], t.qs) + negacyclic(crt(out[i, 1, 0], t.qs), t.s)
            err = [abs(int(v)) for v in centre((value - sigma(t.msg, k)) % t.Q, t.Q)]
            assert max(err) <= bound, (k, max(err), bound)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_reference_really_computes_a_linear_transform(g, bits):
    """out_0 + out_1 s - sum_g pt_g sigma_k(msg), centred mod Q, within (1 + h) / 2 + 1: the bound
    test_it_really_computes_a_linear_transform derives (one ModDown per component, whatever G and the weights are)"""
    t = noiseless_instance(g, bits, np.random.default_rng(29 + bits))
    bound = (1 + int(sum(abs(v) for v in t.s))) / 2 + 1
    want = sum(negacyclic(pt, sigma(t.msg, k)) for pt, k in zip(t.pts, t.elts))
    out = exact_rotate_hoisted_sum(g, t.cases, t.L, bits, t.a, t.c0, t.keys, t.elts, t.weights, False)
    value = crt(out[0, 0], t.qs) + negacyclic(crt(out[1, 0], t.qs), t.s)
    err = [abs(int(v)) for v in centre((value - want) % t.Q, t.Q)]
    assert max(err) <= bound, (max(err), bound)
    # a null weight is 1: the same with the weights left out is the plain sum of the two rotations
    out = exact_rotate_hoisted_sum(g, t.cases, t.L, bits, t.a, t.c0, t.keys, t.elts, [None, None], False)
    plain = exact_rotate_hoisted_sum(g, t.cases, t.L, bits, t.a, t.c0, t.keys, t.elts, None, False)
    assert np.array_equal(out, plain)
    value = crt(out[0, 0], t.qs) + negacyclic(crt(out[1, 0], t.qs), t.s)
    err = [abs(int(v)) for v in centre((value - sum(sigma(t.msg, k) for k in t.elts)) % t.Q, t.Q)]
    assert max(err) <= bound, (max(err), bound)


@pytest.mark.parametrize("bits", [64, 32])
def test_one_identity_element_is_the_exact_inner_product(g, bits):
    """G = 1, k = 1, no c0, no weights: u_0 is innerprod_utils.ref_inner_product, also through key_limbs"""
    n_power, L, K, D, count = 5, 3, 2, 2, 3
    M = L + K
    qs = [c.q for c in host_cases(bits, n_power, WIDE[bits], M)]
    rng = np.random.default_rng(bits)
    for km, limbs in ((M, None), (M + 3, [0, 2, 3, 6, 7])):
        a, key, _ = operands(rng, bits, qs, n_power, D, 2, count, D, km)
        u = exact_u(g, qs, L, n_power, g.X_N_plus, a, None, [key], [1], limbs)
        assert np.array_equal(u[0], ref_inner_product(qs, a, key, None, D, limbs))
