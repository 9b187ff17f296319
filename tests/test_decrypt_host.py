"""KeySwitchPlan.phase / encrypt_public and BfvMultiplyPlan.scale_message / decode without a GPU: decrypt_exact's decode
against Fraction rounding (outside the band the true rounding, inside it that or that - 1, the noise word within 3 L of
2^W v), scale_message against its definition, decode(scale_message(m) + e) = m, the identities that make the outputs a
ciphertext and a phase, and the kernels' own text on CPU threads under AddressSanitizer and UBSan
(tests/cpp/emulate_decrypt.cpp), every word against decrypt_exact."""
import math
from fractions import Fraction

import numpy as np
import pytest

from decrypt_exact import (combine_public, exact_decode, exact_encrypt_public, exact_phase, exact_scale_message,
                           noise_max, phase_words, true_round)
from decrypt_utils import (PLAIN, emulator_job, fresh_x, half_edges, random_x, residues, run_emulator, top_plain, usable)
from hoisted_exact import WIDE, host_cases, transform
from innerprod_utils import from_words, random_words
from keygen_exact import coefficients, exact_lift
from keygen_utils import planted_errors
from keyswitch_utils import centre, crt, negacyclic


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def bases(bits, L):
    """the L widest primes the wide ring helpers give"""
    return [c.q for c in host_cases(bits, 3, WIDE[bits], L)]


def test_symbols_are_exported(g):
    for s in ("u32", "u64"):
        for name in ("keyswitch_plan_phase_scratch_bytes", "keyswitch_plan_phase",
                     "keyswitch_plan_encrypt_public_scratch_bytes", "keyswitch_plan_encrypt_public",
                     "bfv_plan_scale_message", "bfv_plan_decode", "bfv_plan_decode_partials_bytes",
                     "bfv_plan_decode_two_launch", "bfv_plan_decrypt_scratch_bytes", "bfv_plan_decrypt",
                     "bfv_noise_budget_bits"):
            assert "gpuntt_%s_%s" % (name, s) in g.EXPORTED_SYMBOLS
            assert hasattr(g.load_library(), "gpuntt_%s_%s" % (name, s))


def test_noise_budget_bits(g):
    """max(0, W - 1 - bit_length(noise_max + 3 L)), the wrapper and the C ABI alike"""
    lib = g.load_library()
    for bits, fn in ((64, lib.gpuntt_bfv_noise_budget_bits_u64), (32, lib.gpuntt_bfv_noise_budget_bits_u32)):
        for L in (1, 3, 64):
            for v in (0, 1, 5, (1 << (bits // 2)) - 3 * L, (1 << (bits - 2)), (1 << (bits - 1)), (1 << bits) - 1):
                want = max(0, bits - 1 - (v + 3 * L).bit_length())
                assert g.noise_budget_bits(v, L, bits) == want
                assert fn(g._ct(bits)(v), L) == want
    assert g.noise_budget_bits(0, 1, 64) == 61 and g.noise_budget_bits(1 << 63, 1, 64) == 0


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_decode_is_the_true_rounding(bits, L):
    """2000 random and 2000 fresh x per (W, L, t): none in the band (the cap is zero), every message the true rounding,
    |2^W v - n| < 3 L"""
    qs = bases(bits, L)
    Q = math.prod(qs)
    for t in PLAIN[bits]:
        assert usable(t, qs, bits), t
        rng = np.random.default_rng(bits * 1000 + L * 100 + t % 97)
        xs = random_x(rng, Q, 2000) + fresh_x(rng, Q, t, 2000)[0] + [0, Q - 1]
        message, noise, band = exact_decode(qs, t, residues(xs, qs)[None], bits)
        assert not band.any(), (t, int(band.sum()))
        for j, x in enumerate(xs):
            want, v = true_round(x, Q, t)
            assert int(message[0, j]) == want, (t, j)
            assert abs(v * (1 << bits) - int(noise[0, j])) < 3 * L, (t, j)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_inside_the_band_it_is_the_true_rounding_or_one_less(bits, L):
    """planted half-edges x = floor(Q (2 k + 1) / (2 t)) + {0, 1} do hit the band; there and only there the message may be
    the true rounding - 1 (mod t)"""
    qs = bases(bits, L)
    Q = math.prod(qs)
    hits = 0
    for t in PLAIN[bits]:
        rng = np.random.default_rng(bits + L + t % 89)
        xs = half_edges(rng, Q, t, 400)
        message, noise, band = exact_decode(qs, t, residues(xs, qs)[None], bits)
        hits += int(band.sum())
        for j, x in enumerate(xs):
            want, _ = true_round(x, Q, t)
            if band[0, j]:
                assert int(message[0, j]) in (want, (want - 1) % t), (t, j)
            else:
                assert int(message[0, j]) == want, (t, j)
    assert hits > 0


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_scale_message_is_its_definition_and_decodes(bits, L):
    """exact_scale_message = floor((Q m + h) / t) mod q_i for m in {0, 1, t - 1, random} (and for words beyond t, read
    modulo t); decode(scale_message(m) + e) = m for |e| t + t / 2 < Q / 2 - 3 L Q / 2^W, up to the largest such e"""
    qs = bases(bits, L)
    Q = math.prod(qs)
    for t in PLAIN[bits] + [top_plain(qs, bits)]:
        rng = np.random.default_rng(t % 1013 + bits)
        ms = [0, 1, t - 1] + [int(v) for v in rng.integers(0, min(t, 1 << 62), size=60)]
        words = ms + [t, t + 1, (1 << bits) - 1]
        out = exact_scale_message(qs, t, np.array([words], dtype=object))
        for j, w in enumerate(words):
            want = (Q * (w % t) + t // 2) // t
            assert [int(out[0, i, j]) for i in range(L)] == [want % q for q in qs], (t, j)
        # the largest error that still decodes.  t x / Q = m + (e t + h - r) / Q: the scaling's own rounding h - r, at
        # most t / 2 in size, stands beside e t, so the condition is |e| t + t / 2 < Q / 2 - 3 L Q / 2^W (with |e| t alone
        # on the left the claim is false: t = 257, L = 1, u64, e = 8972151786823584 decodes one coefficient to m + 1)
        cap = Fraction(Q, 2) - Fraction(3 * L * Q, 1 << bits) - Fraction(t, 2)
        e_max = int(cap / t)
        if e_max * t >= cap:
            e_max -= 1
        if e_max < 0:  # t as large as Q (L = 1, the top t): the scaling's own rounding already uses the whole margin
            assert L == 1 and t > 1 << (bits - 4)
            continue
        for e in (0, 1, -1, e_max, -e_max, e_max // 2 + 1):
            xs = [((Q * m + t // 2) // t + e) % Q for m in ms]
            message, _, _ = exact_decode(qs, t, residues(xs, qs)[None], bits)
            assert [int(v) for v in message[0]] == ms, (t, e)


@pytest.mark.parametrize("bits", [64, 32])
def test_public_key_encryption_decrypts_to_the_documented_sum(bits):
    """exact_encrypt_public then exact_phase: m + e_pk u + e0 + e1 s (negacyclic, n_power 3), exactly modulo Q; and
    exact_phase with three components is c0 + c1 s + c2 s^2 by CRT"""
    n_power, L, count = 3, 3, 2
    n = 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], L)
    qs = [c.q for c in cases]
    Q = math.prod(qs)
    rng = np.random.default_rng(bits + 5)
    s_small = rng.integers(-1, 2, size=(1, n))
    s = exact_lift(cases, s_small, True)[0]
    s_int = np.array([int(v) for v in s_small[0]], dtype=object)
    # the public key: an encryption of zero, pk0 = e_pk - a s
    e_pk = planted_errors(rng, (1, n), bound=50)
    a = np.stack([rng.integers(0, q, size=n, dtype=np.uint64).astype(object) for q in qs])
    E = exact_lift(cases, e_pk, True)[0]
    pk = np.stack([np.stack([(E[m] - a[m] * s[m]) % q for m, q in enumerate(qs)]), a])
    small = planted_errors(rng, (3, count, n))
    m_int = np.array([[int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)] for _ in range(count)], dtype=object)
    message = transform(cases, np.stack([np.stack([m_int[r] % q for q in qs]) for r in range(count)]), False)
    epk_int = np.array([int(v) for v in e_pk[0]], dtype=object)
    for msg, plain in ((message, m_int), (None, np.zeros((count, n), dtype=object))):
        ct = exact_encrypt_public(cases, pk, small, msg)
        for output_ntt in (True, False):
            ph = exact_phase(cases, ct, s, True, output_ntt)
            for r in range(count):
                value = coefficients(cases, ph[r]) if output_ntt else crt(ph[r], qs)
                u, e0, e1 = (np.array([int(v) for v in small[k, r]], dtype=object) for k in range(3))
                want = plain[r] + negacyclic(epk_int, u) + e0 + negacyclic(e1, s_int)
                assert all(int(v) == 0 for v in (value - want) % Q), (r, output_ntt)

    # three components, coefficient form in and out: c0 + c1 s + c2 s^2 over the integers modulo Q
    c = np.array([[[int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)] for _ in range(count)] for _ in range(3)],
                 dtype=object)
    ct3 = np.stack([np.stack([np.stack([c[k, r] % q for q in qs]) for r in range(count)]) for k in range(3)])
    ph = exact_phase(cases, ct3, s, False, False)
    s2 = negacyclic(s_int, s_int)
    for r in range(count):
        want = c[0, r] + negacyclic(c[1, r], s_int) + negacyclic(c[2, r], s2)
        assert all(int(v) == 0 for v in (crt(ph[r], qs) - want) % Q), r


# (bits, n_power, L, count, off, t, moduli or None for the widest primes of the ring helpers): N = 2 with the one-word
# loader (u32, and u64 off alignment) and with the group of two; N = 32; L = 1 and 3; N = 1024 off alignment has several
# column tiles and lanes past the ring in the last workgroup; moduli beside a power of two (2^61 - 1, 2^31 - 1 below the
# 2^29 - 3 / 2^30 - 35 pair) and a power of two itself, which bc_z stores as R = 0
EMULATED = [(32, 1, 3, 2, 0, 257, None), (64, 1, 3, 3, 0, 65537, None), (64, 1, 1, 2, 1, 2, None),
            (32, 5, 1, 3, 0, (1 << 27) + 1, None), (64, 5, 3, 3, 0, (1 << 59) + 1, None), (64, 5, 3, 2, 1, 257, None),
            (32, 5, 3, 2, 1, 65537, None), (64, 10, 1, 2, 1, (1 << 31) - 1, None),
            (64, 5, 3, 2, 0, 65537, [(1 << 61) - 1, (1 << 62) - 57, 1 << 40]),
            (32, 5, 3, 2, 0, 257, [(1 << 29) - 3, (1 << 30) - 35, 1 << 20])]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(tmp_path):
    """every word of decrypt_phase (2 and 3 components, and in place), encrypt_public_combine (with and without a
    message), bfv_scale_message and bfv_decode (messages and the per-stack maxima, with the half-edges planted) against
    decrypt_exact; the program itself reports a touched guard band or input"""
    rng = np.random.default_rng(23)
    cases, arrays, want = [], [], []
    for bits, n_power, L, count, off, t, mods in EMULATED:
        n = 1 << n_power
        mods = bases(bits, L) if mods is None else mods
        Q = math.prod(mods)
        assert all(t < q and math.gcd(t, q) == 1 for q in mods) and t < 1 << (bits - 2)
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in mods] + mods
        ct = random_words(rng, (3, count, L, n), bits, plant)
        s = random_words(rng, (L, n), bits, plant)
        pk = random_words(rng, (2, L, n), bits, plant)
        lifted = random_words(rng, (3, count, L, n), bits, plant)
        msg = random_words(rng, (count, L, n), bits, plant)
        message = random_words(rng, (count, n), bits, [0, 1, t - 1, t, top])
        x = random_words(rng, (count, L, n), bits, plant)
        edges = half_edges(rng, Q, t, n)  # stack 0: residues of the half-edges, 0 and Q - 1
        edges[0], edges[-1] = 0, Q - 1
        x[0] = residues(edges, mods)
        cases.append((bits, n_power, L, count, off, t, mods))
        arrays.append((ct, s, pk, lifted, msg, message, x))
        dm, dn, _ = exact_decode(mods, t, x, bits)
        p3 = phase_words(mods, ct, s)
        want.append((phase_words(mods, ct[:2], s), p3, p3, combine_public(mods, pk, lifted, msg),
                     combine_public(mods, pk, lifted, None), exact_scale_message(mods, t, message), dm, noise_max(dn),
                     dm, noise_max(dn), dm))
    got, text = run_emulator(tmp_path, emulator_job(cases, arrays))
    assert "vec=0000" in text and "vec=1111" in text, text
    at = 0
    for case, parts in zip(EMULATED, want):
        for k, w in enumerate(parts):
            part = got[at:at + w.size]
            at += w.size
            assert np.array_equal(from_words(part, w.shape), w), (case, k)
    assert at == got.size
