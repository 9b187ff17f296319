"""BFV batching without a GPU: the slot convention of include/gpuntt/rns/bfv_encode.cuh checked by brute force -- pos is
a bijection, the library's host maps equal the model's, the slot values are Horner evaluations at psi^e, sigma_{5^s}
rotates both rows left by s, sigma_{2N-1} swaps them, the negacyclic product is the slot-wise product, and
GPU_Automorphism_NTT's index map agrees -- then the models of lift_centred and multiply_plain at their edges, and the
three kernels' own text on CPU threads under AddressSanitizer and UBSan (tests/cpp/emulate_bfv_encode.cpp), every word
against tests/encode_exact.py."""
import numpy as np
import pytest

from encode_exact import (centre, exact_decode, exact_encode, exact_multiply_plain, horner_slots, lift_centred,
                          negacyclic_product, plain_case, psi_of, rotate_rows, sigma, slot_exponent, slot_maps,
                          slot_position, swap_rows)
from encode_utils import emulator_job, run_emulator
from hoisted_exact import WIDE, host_cases
from innerprod_utils import from_words, random_words

T = 65537


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def test_symbols_are_exported(g):
    for s in ("u32", "u64"):
        for name in ("bfv_encoder_workspace_bytes", "bfv_encoder_scratch_bytes", "bfv_encoder_create",
                     "bfv_encoder_encode", "bfv_encoder_decode", "bfv_encoder_owns_workspace", "bfv_encoder_destroy",
                     "keyswitch_plan_lift_centred", "keyswitch_plan_multiply_plain"):
            assert "gpuntt_%s_%s" % (name, s) in g.EXPORTED_SYMBOLS
    assert "gpuntt_bfv_slot_maps" in g.EXPORTED_SYMBOLS


@pytest.mark.parametrize("n_power", range(1, 17))
def test_pos_is_a_bijection_and_the_library_maps_equal_the_model(g, n_power):
    n = 1 << n_power
    to_position, to_slot = g.bfv_slot_maps(n_power)
    assert sorted(int(v) for v in to_position) == list(range(n))
    assert np.array_equal(to_slot[to_position], np.arange(n, dtype=np.uint32))
    if n_power <= 10:  # the model walks every slot in Python integers
        want_position, want_slot = slot_maps(n_power)
        assert np.array_equal(to_position, want_position) and np.array_equal(to_slot, want_slot)
    else:  # spot checks across both rows
        for slot in (0, 1, 7, n // 2 - 1, n // 2, n // 2 + 5, n - 1):
            assert int(to_position[slot]) == slot_position(slot, n_power), slot


def test_the_host_maps_refuse_what_the_header_says(g):
    for n_power in (0, 29, -1):
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            g.bfv_slot_maps(n_power)
    import ctypes
    assert g.load_library().gpuntt_bfv_slot_maps(0, None, None) != 0
    buf = (ctypes.c_uint32 * 4)()
    assert g.load_library().gpuntt_bfv_slot_maps(2, buf, None) != 0
    assert g.load_library().gpuntt_last_error().decode() == "null pointer argument"


@pytest.mark.parametrize("n_power", [1, 2, 3, 4, 5])
def test_slots_are_horner_evaluations_and_the_three_semantic_facts_hold(g, n_power):
    """decode = a(psi^e) by Horner's rule; encode is its inverse; k = 5^s rotates both rows left by s; 2N - 1 swaps the
    rows; the negacyclic product is the slot-wise product; GPU_Automorphism_NTT's index formula permutes GPU_NTT's order
    accordingly"""
    n = 1 << n_power
    case = plain_case(64, n_power, T)
    psi = psi_of(T, n_power)  # the root plain_case builds the oracle's tables from
    rng = np.random.default_rng(n_power)
    a = rng.integers(0, T, size=(2, n)).astype(object)
    slots = exact_decode(case, a)
    for p in range(2):
        assert np.array_equal(slots[p], horner_slots(a[p], T, psi, n_power)), p
    assert np.array_equal(exact_encode(case, slots), a)
    # any words are read modulo t
    assert np.array_equal(exact_encode(case, slots + T * rng.integers(0, 1000, size=slots.shape).astype(object)), a)
    to_position, to_slot = slot_maps(n_power)
    spectrum = np.zeros((2, n), dtype=object)
    spectrum[:, to_position.astype(np.int64)] = slots
    for s in list(range(-3, 4)) + [n // 2, n]:
        k = g.galois_element_for_rotation(s, n_power)
        assert k == pow(5, s, 2 * n)
        rotated = np.stack([sigma(a[p], k, T) for p in range(2)])
        assert np.array_equal(exact_decode(case, rotated), rotate_rows(slots, s)), s
        src = g.automorphism_index_map(n_power, k, g.X_N_plus).astype(np.int64)
        assert np.array_equal(spectrum[:, src][:, to_position.astype(np.int64)], rotate_rows(slots, s)), s
    k = g.galois_element_for_conjugation(n_power)
    assert k == 2 * n - 1
    swapped = np.stack([sigma(a[p], k, T) for p in range(2)])
    assert np.array_equal(exact_decode(case, swapped), swap_rows(slots))
    src = g.automorphism_index_map(n_power, k, g.X_N_plus).astype(np.int64)
    assert np.array_equal(spectrum[:, src][:, to_position.astype(np.int64)], swap_rows(slots))
    product = negacyclic_product(a[0], a[1], T)[None, :]
    assert np.array_equal(exact_decode(case, product)[0], (slots[0] * slots[1]) % T)
    assert [slot_exponent(s, n_power) for s in (0, n // 2)] == [1, 2 * n - 1]


def test_lift_centred_at_the_edges():
    """m = (t + 1) >> 1 - 1 stays, m = (t + 1) >> 1 becomes negative, m = t - 1 is -1, words of t and beyond are read
    modulo t; t = 2 maps 1 to -1; a t above a limb's modulus is reduced again"""
    for t in (65537, 2, 7, (1 << 61) - 1, (1 << 30) - 35):
        up = (t + 1) >> 1
        words = np.array([0, 1 % t, up - 1, up % t, t - 1, t, t + up - 1, t + up, 3 * t + (t - 1), (1 << 64) - 1],
                         dtype=object)
        v = centre(words, t)
        for w, c in zip(words, v):
            assert (c - w) % t == 0 and -(t // 2) <= c <= t // 2 and (c < (t + 1) // 2), (t, w, c)
        if t > 2:
            assert v[2] == up - 1 and v[3] == up - t and v[4] == -1 and v[5] == 0
        else:
            assert list(v[:5]) == [0, -1, 0, -1, -1]
        qs = [2**62 - 57, 2**31 - 1, 15015, 97, 2]  # the last three lie below the large t
        out = lift_centred(qs, t, words[None, :])
        for i, q in enumerate(qs):
            for j in range(len(words)):
                assert 0 <= out[0, i, j] < q and (out[0, i, j] - v[j]) % q == 0, (t, q, j)


@pytest.mark.parametrize("bits", [64, 32])
def test_multiply_plain_model_on_any_words(bits):
    qs = [c.q for c in host_cases(bits, 3, WIDE[bits], 3)]
    rng = np.random.default_rng(bits)
    top = (1 << bits) - 1
    ct = random_words(rng, (2, 3, 3, 8), bits, [0, top] + qs)
    for pc in (1, 3):
        pt = random_words(rng, (pc, 3, 8), bits, [0, top] + [q - 1 for q in qs])
        ct[:, :, :, 7], pt[:, :, 7] = top, top
        out = exact_multiply_plain(qs, ct, pt)
        for c in range(2):
            for r in range(3):
                for i, q in enumerate(qs):
                    for j in range(8):
                        want = int(ct[c, r, i, j]) * int(pt[r if pc == 3 else 0, i, j]) % q
                        assert out[c, r, i, j] == want


# (bits, n_power, L, K, count, off, slices, t): N = 2 with the one-word loader (u32) and the group of two (u64); every
# operand one word off alignment; N = 512 has two (u64: one, with 256 lanes of two) column tiles; batch slices 1, 2 and
# count; t = 2, 65537, above every modulus of the narrow ring and at the top of the word
EMULATED = [(32, 1, 3, 2, 3, 0, 1, 5), (64, 1, 3, 2, 3, 0, 2, 65537), (64, 1, 3, 2, 3, 1, 3, 2),
            (32, 2, 2, 1, 3, 0, 3, 2), (64, 5, 3, 2, 3, 1, 2, 65537), (32, 5, 3, 2, 3, 1, 1, (1 << 30) - 35),
            (64, 9, 3, 2, 3, 0, 2, (1 << 61) - 1), (32, 9, 3, 2, 2, 0, 2, 65537), (32, 11, 1, 1, 2, 1, 1, 65537)]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(tmp_path):
    """every word of bfv_slot_permute (both directions), lift_centred (both bases) and multiply_plain (shared, per
    ciphertext, in place) against encode_exact; the program itself reports a touched guard band or input"""
    rng = np.random.default_rng(24)
    cases, arrays, want = [], [], []
    for bits, n_power, L, K, count, off, slices, t in EMULATED:
        M, n = L + K, 1 << n_power
        mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], M)]
        top = (1 << bits) - 1
        up = (t + 1) >> 1
        plant = [0, top, t - 1, t, up - 1, up, t + up] + [q - 1 for q in mods] + mods
        plant = [v & top for v in plant]
        values = random_words(rng, (count, n), bits, plant)
        spectrum = random_words(rng, (count, n), bits, plant)
        words = random_words(rng, (count, n), bits, plant)
        ct = random_words(rng, (2, count, L, n), bits, plant)
        pt = random_words(rng, (count, L, n), bits, plant)
        cases.append((bits, n_power, L, K, count, off, slices, t, mods))
        arrays.append((values, spectrum, words, ct, pt))
        to_position, to_slot = slot_maps(n_power)
        per = exact_multiply_plain(mods[:L], ct, pt)
        want.append(((values % t)[:, to_slot.astype(np.int64)], spectrum[:, to_position.astype(np.int64)],
                     lift_centred(mods, t, words), lift_centred(mods[:L], t, words),
                     exact_multiply_plain(mods[:L], ct, pt[:1]), per, per))
    got, text = run_emulator(tmp_path, emulator_job(cases, arrays))
    for flag in ("pvec", "lvec", "mvec"):
        assert " %s=0" % flag in text and " %s=1" % flag in text, text
    at = 0
    for case, parts in zip(EMULATED, want):
        for k, w in enumerate(parts):
            part = got[at:at + w.size]
            at += w.size
            assert np.array_equal(from_words(part, w.shape), w), (case, k)
    assert at == got.size
