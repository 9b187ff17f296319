"""The exact-integer reference of linear_transform_bsgs (tests/bsgs_exact.py, part (c)) checked on its own, no GPU: on a
noiseless instance its output decrypts to sum_g sigma_g(sum_b pt_{g,b} sigma_b(msg)) within the bound
test_gpu_bsgs.test_it_really_computes_the_matrix_product derives, on rings of 62/61-bit and of 30/29-bit primes; the
degenerate call is hoisted_exact.exact_rotate_hoisted_sum word for word; an absent weight is a zero weight and not a one;
and one slot of its accumulator is bsgs_exact.giant_definition (and giant_words, the kernel's word arithmetic) fed the
reference's own digits, keys and v words."""
import math
import os

import numpy as np
import pytest

from bsgs_exact import (exact_baby, exact_bsgs_acc, exact_giant_digits, exact_linear_transform_bsgs, exact_v,
                        giant_definition, giant_words)
from hoisted_exact import WIDE, exact_rotate_hoisted_sum, host_cases, transform
from innerprod_utils import random_words
from keyswitch_utils import centre, crt, negacyclic, partition, ref_mod_up

N_POWER, L, K, ALPHA = 5, 3, 2, 2
M, N = L + K, 1 << N_POWER


def sigma(x, k):
    """a(X) -> a(X^k) in Z[X] / (X^N + 1)"""
    n = len(x)
    out = np.zeros(n, dtype=object)
    for i in range(n):
        e = (i * k) % (2 * n)
        out[e % n] += x[i] if e < n else -x[i]
    return out


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def wide_cases(bits):
    cases = host_cases(bits, N_POWER, WIDE[bits], M)
    assert [c.q.bit_length() for c in cases] == [WIDE[bits][i % 4] for i in range(M)]
    return cases


def any_operands(bits, cases, rng, count, n1, n2, D=2):
    """a, c0, c1, n1 + n2 keys and n2 x n1 weights of arbitrary words, with 0, 2^W - 1, q - 1 and q planted"""
    qs = [c.q for c in cases]
    plant = [0, (1 << bits) - 1] + [q - 1 for q in qs] + qs

    def some(*shape):
        return random_words(rng, shape, bits, plant)
    return dict(a=some(D, count, M, N), c0=some(count, L, N), c1=some(count, L, N),
                bkeys=[some(D, 2, M, N) for _ in range(n1)], gkeys=[some(D, 2, M, N) for _ in range(n2)],
                weights=[[some(M, N) for _ in range(n1)] for _ in range(n2)])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n1,n2", [(2, 2), (3, 3)])
def test_the_reference_really_computes_the_matrix_product(g, bits, n1, n2):
    """The noiseless instance of test_gpu_bsgs.test_it_really_computes_the_matrix_product with every step in Python
    integers and the oracle's transforms: c0 + c1 s = msg (mod Q); the first baby step and the first giant step are the
    identity without a key, every other step has the noiseless key key_k[d] = (-a_d s + P g_d sigma_k(s), a_d); the
    diagonals are small signed integers.  That test's docstring derives the bound: (1 + h) / 2 + 1 for the single final
    ModDown plus h / 2 + 1 per giant step WITH a key (the residue conv_g of V_g1 mod P that its mod_down removes, times
    s, divided by P): (1 + h) / 2 + 1 + n2k (h / 2 + 1), here n2k = n2 - 1 = 1 and 2.  A derivation, not a measurement"""
    rng = np.random.default_rng(29 + bits + n1)
    cases = wide_cases(bits)
    full = [c.q for c in cases]
    qs, ps = full[:L], full[L:]
    Q, P = math.prod(qs), math.prod(ps)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=N)], dtype=object)
    h = int(sum(abs(v) for v in s))
    parts = partition(L, ALPHA)

    def switching_key(k):
        key = np.zeros((len(parts), 2, M, N), dtype=object)
        for d, S in enumerate(parts):
            Qd = math.prod(qs[i] for i in S)
            gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
            a_d = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(N)], dtype=object)
            b_d = -negacyclic(a_d, s) + P * gd * sigma(s, k)
            for m, q in enumerate(full):
                key[d, 0, m], key[d, 1, m] = b_d % q, a_d % q
        return transform(cases, key, False)

    def ntt_form(x, sub):
        return transform(sub, np.array([x % c.q for c in sub], dtype=object), False)

    rot = [g.galois_element_for_rotation(r, N_POWER) for r in (1, 2, 3, 6)]
    belts, gelts = ([1, rot[0]], [1, rot[1]]) if n1 == 2 else ([1, rot[0], rot[1]], [1, rot[2], rot[3]])
    bkeys = [None] + [switching_key(k) for k in belts[1:]]
    gkeys = [None] + [switching_key(k) for k in gelts[1:]]
    pts = [[np.array([int(v) for v in rng.integers(-50, 51, size=N)], dtype=object) for _ in range(n1)]
           for _ in range(n2)]
    weights = [[ntt_form(pt, cases) for pt in row] for row in pts]
    c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(N)], dtype=object)
    msg = np.array([int(v) for v in rng.integers(-1000, 1000, size=N)], dtype=object)
    c0 = (msg - negacyclic(c1, s)) % Q
    a = transform(cases, ref_mod_up(qs, ps, ALPHA, np.array([[c1 % q for q in qs]], dtype=object), bits, True), False)
    d_c0, d_c1 = ntt_form(c0, cases[:L])[None], ntt_form(c1, cases[:L])[None]
    want = sum(sigma(sum(negacyclic(pts[gi][b], sigma(msg, kb)) for b, kb in enumerate(belts)), kg)
               for gi, kg in enumerate(gelts))
    bound = (1 + h) / 2 + 1 + (n2 - 1) * (h / 2 + 1)
    for output_ntt in (False, True):
        out = exact_linear_transform_bsgs(g, cases, L, ALPHA, bits, a, d_c0, d_c1, bkeys, belts, gkeys, gelts, weights,
                                          output_ntt)
        assert out.shape == (2, 1, L, N)
        if output_ntt:
            out = transform(cases[:L], out, True)
        value = crt(out[0, 0], qs) + negacyclic(crt(out[1, 0], qs), s)
        err = [abs(int(v)) for v in centre((value - want) % Q, Q)]
        print("largest error %d, bound %.1f" % (max(err), bound))
        assert max(err) <= bound, (max(err), bound)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_degenerate_call_is_the_reference_of_rotate_hoisted_sum(g, bits):
    """n2 = 1, a giant step without a key, every baby key and every weight present: exact_rotate_hoisted_sum's words"""
    cases, rng, count, n1 = wide_cases(bits), np.random.default_rng(bits), 2, 4
    t = any_operands(bits, cases, rng, count, n1, 1)
    belts = [g.galois_element_for_rotation(1, N_POWER), 1, g.galois_element_for_conjugation(N_POWER),
             g.galois_element_for_rotation(1, N_POWER)]
    for c0, output_ntt in ((t["c0"], False), (None, True)):
        out = exact_linear_transform_bsgs(g, cases, L, ALPHA, bits, t["a"], c0, None, t["bkeys"], belts, [None], [1],
                                          t["weights"], output_ntt)
        want = exact_rotate_hoisted_sum(g, cases, L, bits, t["a"], c0, t["bkeys"], belts, t["weights"][0], output_ntt)
        assert np.array_equal(out, want)


@pytest.mark.parametrize("bits", [64, 32])
def test_a_null_weight_is_absent_not_one(g, bits):
    cases, rng, count, n1, n2 = wide_cases(bits), np.random.default_rng(1 + bits), 2, 3, 2
    t = any_operands(bits, cases, rng, count, n1, n2)
    belts = [g.galois_element_for_rotation(1, N_POWER), 1, g.galois_element_for_rotation(-1, N_POWER)]
    gelts = [g.galois_element_for_rotation(3, N_POWER), 1]
    bkeys, gkeys = [t["bkeys"][0], None, t["bkeys"][2]], [t["gkeys"][0], None]

    def run(w01, w12):
        weights = [[t["weights"][0][0], w01, t["weights"][0][2]], [t["weights"][1][0], t["weights"][1][1], w12]]
        return exact_linear_transform_bsgs(g, cases, L, ALPHA, bits, t["a"], t["c0"], t["c1"], bkeys, belts, gkeys, gelts,
                                           weights, True)
    zero, one = np.zeros((M, N), dtype=object), np.ones((M, N), dtype=object)
    absent = run(None, None)
    assert np.array_equal(absent, run(zero, zero))
    assert not np.array_equal(absent, run(one, None)) and not np.array_equal(absent, run(None, one))


@pytest.mark.parametrize("bits", [64, 32])
def test_one_slot_of_the_accumulator_is_the_giant_definition(g, bits):
    """acc[c][r][m][j] of the reference against bsgs_exact.giant_definition -- the per-step canonical sums
    tests/test_bsgs_host.py pins the kernel's word arithmetic to -- and giant_words, fed the reference's own digits
    a'_g[d][r][m][pi_g(j)], the key words at j (any words: read modulo q_m), v_g[0] at pi_g(j) for the keyed steps and
    v_g[c] at j for the steps without a key"""
    cases, rng, count, n1, n2 = wide_cases(bits), np.random.default_rng(2 + bits), 2, 3, 4
    qs = [c.q for c in cases]
    t = any_operands(bits, cases, rng, count, n1, n2)
    belts = [1, g.galois_element_for_rotation(1, N_POWER), g.galois_element_for_rotation(2, N_POWER)]
    gelts = [g.galois_element_for_rotation(3, N_POWER), 1, g.galois_element_for_conjugation(N_POWER), 1]
    bkeys, gkeys = [None] + t["bkeys"][1:], [t["gkeys"][0], None, t["gkeys"][2], None]
    acc = exact_bsgs_acc(g, cases, L, ALPHA, bits, t["a"], t["c0"], t["c1"], bkeys, belts, gkeys, gelts, t["weights"])
    u = exact_baby(g, cases, L, t["a"], t["c0"], t["c1"], bkeys, belts)
    v = [exact_v(qs, u, row) for row in t["weights"]]
    digits = {gi: exact_giant_digits(cases, L, ALPHA, bits, v[gi][1]) for gi in (0, 2)}
    pi = {gi: g.automorphism_index_map(N_POWER, gelts[gi], cases[0].poly).astype(np.int64) for gi in (0, 2)}
    for c, r, m, j in ((0, 0, 0, 0), (0, 1, L - 1, 7), (0, 0, M - 1, N - 1), (1, 1, 1, 13), (1, 0, L, 30)):
        q = qs[m]
        dig = [[int(digits[gi][d, r, m, pi[gi][j]]) for d in range(2)] for gi in (0, 2)]
        key = [[int(gkeys[gi][d, c, m, j]) for d in range(2)] for gi in (0, 2)]
        v0 = [int(v[gi][0, r, m, pi[gi][j]]) if c == 0 else 0 for gi in (0, 2)]
        plain = [int(v[gi][c, r, m, j]) for gi in (1, 3)]
        assert int(acc[c, r, m, j]) == giant_definition(dig, key, v0, plain, q), (c, r, m, j)
        assert int(acc[c, r, m, j]) == giant_words(dig, key, v0, plain, q, bits), (c, r, m, j)
