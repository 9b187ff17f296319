"""BfvMultiplyPlan without a GPU (include/gpuntt/rns/bfv_multiply.cuh): the host references and the constants against
Python integers (bfv_exact), the definition against the ideal value round(t D / Q) and against a decryption -- both in
Python integers alone, so the convention is pinned before a device sees it -- the refusals that need no device, and the
kernels' own text on CPU threads under AddressSanitizer and UBSan (tests/cpp/emulate_bfv.cpp)."""
import math

import numpy as np
import pytest

from bfv_exact import (exact_extend, exact_multiply, exact_scale_round, ideal, in_band, integer_tensor,
                       representatives)
from bfv_utils import aux_count, run_emulator
from hoisted_exact import NARROW, WIDE, host_cases
from innerprod_utils import from_words, random_words, words
from keyswitch_utils import centre, crt, negacyclic


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def bases(bits, n_power, widths, L, t, extra=0, odd=False):
    """NTT primes of the widths: the q-base and the smallest auxiliary base for t (plus `extra` primes; odd: one more
    where that makes K odd), with the cases"""
    cases = host_cases(bits, n_power, widths, 2 * L + 4 + extra)
    mods = [c.q for c in cases]
    K = aux_count(mods, L, t, 1 << n_power) + extra
    K += 1 if odd and K % 2 == 0 else 0
    return mods[:L], mods[L:L + K], cases[:L + K]


def rand_mod(rng, Q):
    """a uniform integer below Q"""
    return sum(int(rng.integers(0, 1 << 62)) << (62 * i) for i in range(Q.bit_length() // 62 + 2)) % Q


def residues(v, mods):
    """an object array of integers -> [len(mods)][...] canonical residues"""
    return np.stack([v % m for m in mods])


def planted(rng, bits, qs, shape, t=1):
    """any words [stacks][L][N] with 0, 2^W - 1, q - 1 and q planted in every limb, and the columns of stack 0 set to the
    values Q/2 - 1, Q/2, Q/2 + 1 (divided by t modulo Q: scale_round multiplies by it)"""
    top, Q = (1 << bits) - 1, math.prod(qs)
    x = random_words(rng, shape, bits, [0, top] + [q - 1 for q in qs] + list(qs))
    n = shape[2]
    for i, q in enumerate(qs):
        for k, v in enumerate((0, top, q - 1, q)):
            x[-1, i, (k + i) % n] = v
    if math.gcd(t, Q) == 1:
        for k, v in enumerate((Q // 2 - 1, Q // 2, Q // 2 + 1)):
            x[0, :len(qs), k % n] = [(v * pow(t, -1, Q)) % Q % q for q in qs]
    return x


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("widths", ["wide", "narrow"])
@pytest.mark.parametrize("n_power", [1, 5])
@pytest.mark.parametrize("stacks", [1, 3])
def test_host_references_against_python_integers(g, bits, widths, n_power, stacks):
    L, t, n = 3, 65537, 1 << n_power
    # narrow: NARROW's width and the three above it (too few NTT primes of 20 bits exist for a whole base)
    narrow = tuple(NARROW[bits][0] + i for i in range(4))
    qs, bs, _ = bases(bits, n_power, WIDE[bits] if widths == "wide" else narrow, L, t)
    M, dt = L + len(bs), g.np_dtype(bits)
    rng = np.random.default_rng(bits + n_power + stacks)
    x = planted(rng, bits, qs, (stacks, L, n))
    got = g.bfv_reference_extend(qs, bs, words(g, x, bits), np.zeros(stacks * M * n, dtype=dt), n_power, stacks, bits)
    assert np.array_equal(from_words(got, (stacks, M, n)), exact_extend(qs, bs, x, bits))
    full = planted(rng, bits, qs + bs, (stacks, M, n), t)
    got = g.bfv_reference_scale_round(qs, bs, t, words(g, full, bits), np.zeros(stacks * L * n, dtype=dt), n_power,
                                      stacks, bits)
    assert np.array_equal(from_words(got, (stacks, L, n)), exact_scale_round(qs, bs, t, full, bits))
    if n_power == 5:  # of the planted columns Q/2 - 1, Q/2, Q/2 + 1 the last one lies in the band (Q is odd)
        assert in_band(qs, bs, t, full, bits)[0, :3].tolist() == [False, False, True]


@pytest.mark.parametrize("bits,t", [(64, (1 << 40) + 15), (32, 257)])
def test_constants_against_python_integers(g, bits, t):
    L, n_power = 3, 4
    qs, bs, _ = bases(bits, n_power, WIDE[bits], L, t)
    K, Q, B, W = len(bs), math.prod(qs), math.prod(bs), bits
    c = g.bfv_constants(qs, bs, t, n_power, bits)
    for side, ins, outs, P in (("up_", qs, bs, Q), ("down_", bs, qs, B)):
        ref = g.baseconv_constants(ins, outs, bits)
        for name, arr in ref.items():
            assert np.array_equal(c[side + name], arr), side + name
        assert [int(v) for v in c[side + "qhat_inv"]] == [pow(P // q, -1, q) for q in ins]
        assert [int(v) for v in c[side + "q_inv_mod_p"]] == [pow(P, -1, p) for p in outs]
        assert [[int(v) for v in row] for row in c[side + "matrix"]] == [[(P // q) % p for p in outs] for q in ins]
    assert [int(v) for v in c["t_mod"]] == [t % m for m in qs + bs]
    assert [int(v) for v in c["t_mod_shoup"]] == [((t % m) << W) // m for m in qs + bs]
    wt = [t * pow(Q // q, -1, q) % q for q in qs]
    assert [int(v) for v in c["t_qhat_inv"]] == wt
    assert [int(v) for v in c["t_qhat_inv_shoup"]] == [(w << W) // q for w, q in zip(wt, qs)]
    assert B >= 2 * t * (1 << n_power) * Q > B // max(bs) and len(bs) == K


# (bits, L, n_power, t, count): the shapes of the prototype, and L = 17 -- K > 16, both conversions cross a 16-term chunk
IDEAL_SHAPES = [(32, 1, 1, 257, 1), (32, 3, 2, 65537, 1), (64, 1, 2, 257, 2), (64, 2, 3, 65537, 1),
                (64, 4, 2, (1 << 40) + 15, 1), (64, 6, 1, (1 << 32) + 15, 2), (64, 17, 1, 65537, 1)]


@pytest.mark.parametrize("bits,L,n_power,t,count", IDEAL_SHAPES)
def test_the_definition_is_the_rounded_scaled_tensor(bits, L, n_power, t, count):
    """Python integers alone: extend, the integer tensor D of the representatives it chose, the residues of D in the full
    base, scale_round -- against round(t D / Q) mod q_i at every coefficient outside step 2's band"""
    n = 1 << n_power
    qs, bs, _ = bases(bits, n_power, WIDE[bits], L, t)
    Q = math.prod(qs)
    rng = np.random.default_rng(bits + L + n_power)
    reps = []
    for _ in range(2):
        v = np.array([rand_mod(rng, Q) for _ in range(2 * count * n)], dtype=object).reshape(2 * count, n)
        for k, c in enumerate((Q // 2 - 1, Q // 2, Q // 2 + 1)):  # planted at the edge of the centred range
            v[k % (2 * count), k % n] = c
        full = exact_extend(qs, bs, np.moveaxis(residues(v, qs), 0, 1), bits)
        rep = representatives(qs, bs, full)
        assert all(abs(int(r)) * (1 << bits) <= Q * ((1 << (bits - 1)) + 3 * L) for r in rep.reshape(-1))
        assert np.array_equal(rep % Q, v)
        reps.append(rep.reshape(2, count, n))
    D = integer_tensor(*reps).reshape(3 * count, n)
    stack = np.moveaxis(residues(D, qs + bs), 0, 1)
    out = exact_scale_round(qs, bs, t, stack, bits)
    band = in_band(qs, bs, t, stack, bits)
    want = np.moveaxis(residues(ideal(t, D, Q), qs), 0, 1)
    keep = ~band
    assert band.sum() * 1000 <= band.size, "more than 0.1 % of the coefficients lie in the rounding band"
    assert np.array_equal(out[np.broadcast_to(keep[:, None, :], out.shape)],
                          want[np.broadcast_to(keep[:, None, :], want.shape)])
    # inside the band the definition is the ideal value or one beside it
    diff = centre((crt(np.moveaxis(out, 1, 0), qs) - ideal(t, D, Q)) % Q, Q)
    assert all(abs(int(d)) <= 1 for d in diff.reshape(-1))


def test_the_three_components_decrypt_to_the_product():
    """Python integers alone: ternary secret, noise in {-1, 0, 1}, Delta = floor(Q / t), Q >= 2^80; the definition's
    three components decrypt under (1, s, s^2) to m1 m2 mod (t, X^N + 1)"""
    bits, L, n_power, t, count = 64, 2, 4, 257, 1
    n = 1 << n_power
    qs, bs, cases = bases(bits, n_power, WIDE[bits], L, t)
    Q = math.prod(qs)
    assert Q >= 1 << 80
    rng = np.random.default_rng(4)
    s = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
    delta = Q // t

    def encrypt(m):
        a = np.array([rand_mod(rng, Q) for _ in range(n)], dtype=object)
        e = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
        c0 = (delta * m + e - negacyclic(a, s)) % Q
        return np.stack([np.moveaxis(residues(c, qs), 0, 1) for c in (c0.reshape(1, n), a.reshape(1, n))])

    m1 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    m2 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    out, _ = exact_multiply(cases, L, t, bits, encrypt(m1), encrypt(m2), False, False)
    d = [crt(np.moveaxis(out[c], 1, 0), qs)[0] for c in range(3)]
    s2 = negacyclic(s, s)
    v = centre((d[0] + negacyclic(d[1], s) + negacyclic(d[2], s2)) % Q, Q)
    got = ((2 * t * v + Q) // (2 * Q)) % t
    assert np.array_equal(got, negacyclic(m1, m2) % t)


def test_refusals_that_need_no_device(g):
    bits, L, n_power, t = 64, 3, 5, 65537
    qs, bs, _ = bases(bits, n_power, WIDE[bits], L, t, extra=1)
    g.bfv_constants(qs, bs[:-1], t, n_power, bits)  # the smallest base passes
    with pytest.raises(ValueError, match="Auxiliary base too small!"):
        g.bfv_constants(qs, bs[:-2], t, n_power, bits)
    many = [c.q for c in host_cases(bits, 1, (60,), 66)]
    refused = [lambda: g.bfv_constants(qs, bs, t, 0, bits), lambda: g.bfv_constants(qs, bs, t, 29, bits),
               lambda: g.bfv_constants(qs, bs[:-1] + [qs[0]], t, n_power, bits),      # not coprime: a q among the b
               lambda: g.bfv_constants(qs[:2] + [qs[0]], bs, t, n_power, bits),       # a q twice
               lambda: g.bfv_constants(qs, bs[:-1] + [bs[0]], t, n_power, bits),      # a b twice
               lambda: g.bfv_constants([], bs, t, n_power, bits),                     # L < 1
               lambda: g.bfv_constants(qs, [], t, n_power, bits),                     # K < 1
               lambda: g.bfv_constants(many[:30], many[30:65], t, 1, bits),           # M > 64
               lambda: g.bfv_constants(qs, bs, 1, n_power, bits),                     # t < 2
               lambda: g.bfv_constants(qs, bs, 0, n_power, bits),
               lambda: g.bfv_constants(qs[:2] + [1], bs, t, n_power, bits),            # "Invalid modulus!"
               lambda: g.bfv_reference_extend(qs, bs, None, np.zeros(8, dtype=np.uint64), 1, 1, bits),
               lambda: g.bfv_reference_scale_round(qs, bs, t, np.zeros(64, dtype=np.uint64), None, 1, 1, bits),
               lambda: g.bfv_reference_extend(qs, bs, np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64), 1,
                                              -1, bits)]
    for i, f in enumerate(refused):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError, match="Invalid n_power range!"):
        g.bfv_constants(qs, bs, t, 29, bits)
    x = np.zeros(2 * (L + len(bs)) * 2, dtype=np.uint64)
    with pytest.raises(ValueError, match="overlap"):  # in inside full
        g.bfv_reference_extend(qs, bs, x[2:], x, 1, 2, bits)


# (bits, n_power, L, K odd, stacks, count, t, off): N = 2 with the one-word loader at u32 and one word off alignment;
# a ragged BC_KB block (K forced odd); several column tiles (N = 256, three stacks); L = 17, K > 16; L = 3 mixes a narrow
# prime with the widest ones
EMULATED = [(32, 1, 1, False, 1, 1, 257, 0), (32, 2, 3, False, 3, 2, 65537, 1), (32, 8, 2, True, 3, 1, 257, 0),
            (64, 1, 3, False, 2, 3, (1 << 40) + 15, 0), (64, 1, 2, False, 1, 1, 257, 1),
            (64, 5, 5, True, 3, 2, 65537, 1), (64, 8, 3, False, 3, 1, 65537, 0), (64, 2, 17, False, 2, 1, 257, 0)]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(g, tmp_path):
    """every word of bfv_extend, bfv_scale_round and bfv_tensor (two operands, and the squaring in place) against
    bfv_exact; the program itself reports a touched guard band"""
    rng = np.random.default_rng(6)
    job, want = [len(EMULATED)], []
    for bits, n_power, L, odd, stacks, count, t, off in EMULATED:
        n = 1 << n_power
        qs, bs, _ = bases(bits, n_power, WIDE[bits] if L != 3 else NARROW[bits] + WIDE[bits], L, t, odd=odd)
        assert len(bs) % 2 == 1 or not odd
        mods, M = qs + bs, L + len(bs)
        x = planted(rng, bits, qs, (stacks, L, n))
        full = planted(rng, bits, mods, (stacks, M, n), t)
        xe, ye = (random_words(rng, (2, count, M, n), bits, [0, (1 << bits) - 1] + mods) for _ in range(2))
        job += [bits, n_power, L, len(bs), stacks, count, t, off] + mods
        for a in (x, full, xe, ye):
            job += [int(v) for v in a.reshape(-1)]

        def tensor(a, b):
            d = np.zeros((3, count, M, n), dtype=object)
            for m, q in enumerate(mods):
                d[0, :, m] = a[0, :, m] * b[0, :, m] % q
                d[1, :, m] = (a[0, :, m] * b[1, :, m] + a[1, :, m] * b[0, :, m]) % q
                d[2, :, m] = a[1, :, m] * b[1, :, m] % q
            return d
        want.append((exact_extend(qs, bs, x, bits), exact_scale_round(qs, bs, t, full, bits), tensor(xe, ye),
                     tensor(xe, xe)))
    path = tmp_path / "job.bin"
    np.array(job, dtype=np.uint64).tofile(path)
    got = np.fromfile(run_emulator(tmp_path, path), dtype=np.uint64)
    at = 0
    for case, arrays in zip(EMULATED, want):
        for k, w in enumerate(arrays):
            part = got[at:at + w.size]
            at += w.size
            assert np.array_equal(from_words(part, w.shape), w), (case, k)
    assert at == got.size
