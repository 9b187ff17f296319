"""KeySwitchPlan.lift_small / generate_keys / encrypt_symmetric without a GPU: keygen_exact against a literal composition
of the public host pieces that existed before it, the identity that makes its output a switching key --
key0 + key1 s = e_d + P g_d s_from (mod P Q) in coefficient form, for every digit -- the same for a ciphertext, and the
kernels' own text on CPU threads under AddressSanitizer and UBSan (tests/cpp/emulate_keygen.cpp), every word against
keygen_exact."""
import math

import numpy as np
import pytest

from hoisted_exact import WIDE, host_cases, transform
from innerprod_utils import from_words, random_words, words
from keygen_exact import (EDGES, coefficients, combine_encrypt, combine_keys, digit_limbs, exact_encrypt,
                          exact_generate_keys, exact_lift, gadget, lift)
from keygen_utils import emulator_job, planted_errors, run_emulator
from keyswitch_utils import centre, crt, negacyclic


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def test_symbols_are_exported(g):
    for s in ("u32", "u64"):
        for name in ("lift_small", "keygen_scratch_bytes", "encrypt_scratch_bytes", "generate_keys", "encrypt_symmetric"):
            assert "gpuntt_keyswitch_plan_%s_%s" % (name, s) in g.EXPORTED_SYMBOLS


def test_lift_edges():
    """the canonical residue of every edge value, also under a modulus below 2^31 and a composite"""
    qs = [2**62 - 57, 2**31 - 1, 15015, 2]
    out = lift(qs, np.array([EDGES], dtype=np.int64))
    for m, q in enumerate(qs):
        for j, v in enumerate(EDGES):
            assert 0 <= out[0, m, j] < q and (out[0, m, j] - v) % q == 0


@pytest.mark.parametrize("bits", [64, 32])
def test_the_model_equals_a_composition_of_the_public_host_pieces(g, bits):
    """key0 of digit d as ONE InnerProductPlan::reference call with three digits -- E * 1 + (q - a) * s + s_from * (P mod
    q_m on the limbs of digit d, 0 elsewhere) -- with P mod q_m from keyswitch_constants: nothing of keygen_exact's
    arithmetic"""
    n_power, L, K, alpha, G = 3, 5, 2, 2, 2
    M, n = L + K, 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], M)
    qs = [c.q for c in cases]
    rng = np.random.default_rng(bits)
    D = len(digit_limbs(L, alpha))
    top = (1 << bits) - 1
    s = random_words(rng, (M, n), bits, [0, top])
    s_from = random_words(rng, (G, M, n), bits, [0, top] + qs)
    a = random_words(rng, (G, D, M, n), bits, [0, top] + qs + [q - 1 for q in qs])
    errors = planted_errors(rng, (G, D, n))
    got = exact_generate_keys(cases, L, alpha, s, s_from, errors, a)
    E = exact_lift(cases, errors, True)
    p_mod_q = [int(v) for v in g.keyswitch_constants(qs[:L], qs[L:], alpha, bits=bits)["down_p_mod_q"]]
    for d, S in enumerate(digit_limbs(L, alpha)):
        neg_a = np.stack([(q - a[:, d, m, :] % q) % q for m, q in enumerate(qs)], axis=1)
        stack = np.stack([E[:, d], neg_a, s_from])  # [3][G][M][N]
        mask = np.zeros((M, n), dtype=object)
        for m in S:
            mask[m, :] = p_mod_q[m]
        key = np.stack([np.ones((M, n), dtype=object), s, mask])[:, None]  # [3][1][M][N]
        out = np.zeros(G * M * n, dtype=g.np_dtype(bits))
        g.innerprod_reference(qs, words(g, stack, bits), words(g, key, bits), out, n_power, 3, 1, G, bits=bits)
        assert np.array_equal(from_words(out, (G, M, n)), got[:, d]), d


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (5, 2, 2)])
def test_the_output_is_a_switching_key(bits, L, K, alpha):
    """in coefficient form, modulo P Q: key0 + key1 s = e_d + P g_d s_from for every digit (the last one ragged)"""
    n_power = 3
    M, n = L + K, 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], M)
    qs = [c.q for c in cases]
    PQ = math.prod(qs)
    rng = np.random.default_rng(7 * bits + L)
    s_small = rng.integers(-1, 2, size=(1, n))
    from_small = rng.integers(-1, 2, size=(2, n))
    s = exact_lift(cases, s_small, True)[0]
    s_from = exact_lift(cases, from_small, True)
    D = len(digit_limbs(L, alpha))
    assert D == -(-L // alpha) and len(digit_limbs(L, alpha)[-1]) == (L - 1) % alpha + 1
    a = np.stack([np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64).astype(object) for q in qs])
                            for _ in range(D)]) for _ in range(2)])
    errors = planted_errors(rng, (2, D, n))
    key0 = exact_generate_keys(cases, L, alpha, s, s_from, errors, a)
    s_int = np.array([int(v) for v in s_small[0]], dtype=object)
    for i in range(2):
        f_int = np.array([int(v) for v in from_small[i]], dtype=object)
        for d, Pg in enumerate(gadget(qs, L, alpha)):
            left = coefficients(cases, key0[i, d]) + negacyclic(coefficients(cases, a[i, d]), s_int)
            right = np.array([int(v) for v in errors[i, d]], dtype=object) + Pg * f_int
            assert all(int(v) == 0 for v in (left - right) % PQ), (i, d)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_ciphertext_decrypts_exactly(bits):
    """c0 + c1 s = e + m (mod Q), exactly; with no message an encryption of zero"""
    n_power, L, K, count = 3, 3, 2, 2
    n = 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], L + K)
    qs = [c.q for c in cases][:L]
    Q = math.prod(qs)
    rng = np.random.default_rng(bits + 1)
    s_small = rng.integers(-1, 2, size=(1, n))
    s = exact_lift(cases, s_small, True)[0]
    s_int = np.array([int(v) for v in s_small[0]], dtype=object)
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64).astype(object) for q in qs])
                  for _ in range(count)])
    errors = planted_errors(rng, (count, n))
    m_int = np.array([[int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)] for _ in range(count)], dtype=object)
    message = transform(cases[:L], np.stack([np.stack([m_int[r] % q for q in qs]) for r in range(count)]), False)
    for msg, plain in ((message, m_int), (None, np.zeros((count, n), dtype=object))):
        c0 = exact_encrypt(cases, L, s, errors, msg, a)
        for r in range(count):
            value = coefficients(cases[:L], c0[r]) + negacyclic(coefficients(cases[:L], a[r]), s_int)
            want = np.array([int(v) for v in errors[r]], dtype=object) + plain[r]
            assert all(int(v) == 0 for v in (value - want) % Q), r
            if msg is None:  # centred, the noise itself
                assert [int(v) for v in centre(value % Q, Q)] == [int(v) for v in errors[r]]


# (bits, n_power, L, K, alpha, keys, off): N = 2 with the one-word loader (u32) and with the group of two (u64); every
# operand one word off alignment; N = 512 one word off alignment has two column tiles; keys 1, 3 and 64; 20 digits; the
# ragged last digit (L = 5, alpha = 2); alpha = 4 = L (one digit)
EMULATED = [(32, 1, 3, 2, 2, 1, 0), (64, 1, 3, 2, 2, 3, 0), (64, 1, 3, 2, 2, 64, 1), (32, 2, 5, 2, 2, 3, 0),
            (64, 5, 5, 3, 2, 3, 1), (32, 6, 4, 1, 4, 1, 1), (64, 9, 3, 2, 1, 1, 1), (32, 9, 3, 2, 2, 3, 0),
            (64, 2, 20, 2, 1, 3, 0)]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(tmp_path):
    """every word of lift_small (both bases) and of keygen_combine (keys; ciphertexts with and without a message)
    against keygen_exact; the program itself reports a touched guard band or `a` plane"""
    rng = np.random.default_rng(22)
    cases, arrays, want = [], [], []
    for bits, n_power, L, K, alpha, keys, off in EMULATED:
        M, n, D = L + K, 1 << n_power, -(-L // alpha)
        mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], M)]
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in mods] + mods
        errors = planted_errors(rng, (keys, D, n))
        e = random_words(rng, (keys, D, M, n), bits, plant)
        s = random_words(rng, (M, n), bits, plant)
        s_from = random_words(rng, (keys, M, n), bits, plant)
        a = random_words(rng, (keys, D, M, n), bits, plant)
        ee = random_words(rng, (keys, L, n), bits, plant)
        ea = random_words(rng, (keys, L, n), bits, plant)
        msg = random_words(rng, (keys, L, n), bits, plant)
        cases.append((bits, n_power, L, K, alpha, keys, off, mods))
        arrays.append((errors, e, s, s_from, a, ee, ea, msg))
        flat = errors.reshape(keys * D, n)
        want.append((lift(mods, flat), lift(mods[:L], flat), combine_keys(mods, L, alpha, e, s, s_from, a),
                     combine_encrypt(mods, L, ee, s, msg, ea), combine_encrypt(mods, L, ee, s, None, ea)))
    got, text = run_emulator(tmp_path, emulator_job(cases, arrays))
    assert " vec=0" in text and " vec=1" in text and "lvec=0" in text and "lvec=1" in text, text
    at = 0
    for case, parts in zip(EMULATED, want):
        for k, w in enumerate(parts):
            part = got[at:at + w.size]
            at += w.size
            assert np.array_equal(from_words(part, w.shape), w), (case, k)
    assert at == got.size
