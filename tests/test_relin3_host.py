"""KeySwitchPlan.mod_down_add / relinearize and BfvMultiplyPlan.multiply_relinearize without a GPU: the entry points and
the refusals that need no device, relin3_exact's two forms of relinearize against each other in Python integers alone (the
fold of P c01 before the ModDown and the addend after it equal the definition), and the kernels' own text on CPU threads
under AddressSanitizer and UBSan (tests/cpp/emulate_relin3.cpp), every word against relin3_exact."""
import ctypes
import itertools

import numpy as np
import pytest

from hoisted_exact import WIDE, host_cases
from innerprod_utils import from_words, random_words
from relin3_exact import exact_definition, exact_mod_down_add, exact_relinearize, exact_seeded
from relin3_utils import emulator_job, run_emulator


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def test_entry_points_refuse_null_pointers_without_a_device(g):
    lib = g.load_library()
    word = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    for s in ("u32", "u64"):
        down = getattr(lib, "gpuntt_keyswitch_plan_mod_down_add_" + s)
        relin = getattr(lib, "gpuntt_keyswitch_plan_relinearize_" + s)
        bfv = getattr(lib, "gpuntt_bfv_plan_multiply_relinearize_" + s)
        assert down(None, p, p, p, 1, None) != 0
        assert relin(None, p, p, p, p, 1, 0, 0, p, None) != 0
        assert bfv(None, p, p, p, p, p, 1, 0, 0, p, p, None) != 0
        assert bfv(p, p, p, None, p, p, 1, 0, 0, p, p, None) != 0  # no key-switching plan


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 4])
def test_what_runs_equals_the_definition_in_python_integers(bits, n_power):
    """all four form combinations, c01 of any words, on the widest primes"""
    L, K, alpha, count = 3, 2, 2, 2
    M, n = L + K, 1 << n_power
    cases = host_cases(bits, n_power, WIDE[bits], M)
    qs = [c.q for c in cases]
    rng = np.random.default_rng(bits + n_power)
    top = (1 << bits) - 1
    c01 = random_words(rng, (2, count, L, n), bits, [0, top] + [q - 1 for q in qs[:L]] + qs[:L])
    key = random_words(rng, (2, 2, M, n), bits, [0, top])
    for input_ntt, output_ntt in itertools.product((False, True), repeat=2):
        c2 = random_words(rng, (count, L, n), bits, [0, top])
        if input_ntt:
            c2 = np.stack([c2[:, m, :] % q for m, q in enumerate(qs[:L])], axis=1)
        want = exact_definition(cases, L, alpha, bits, c01, c2, key, input_ntt, output_ntt)
        got = exact_relinearize(cases, L, alpha, bits, c01, c2, key, input_ntt, output_ntt)
        assert np.array_equal(got, want), (input_ntt, output_ntt)


# (bits, n_power, L, K, alpha, count, off, split): N = 2 with the one-word loader (u32, and u64 one word off alignment);
# L = 6, 5 and 3 leave a ragged BC_KB block in mod_down_add; N = 512 one word off alignment has two column tiles in the
# inner product and 2 count N / 128 in mod_down_add; count 3 and 5 are blocks of 2 and 4 inputs with a ragged tail; the
# output split over 1, 2 and 3 workgroups (3 does not divide the blocks evenly)
EMULATED = [(32, 1, 3, 2, 2, 1, 0, 1), (64, 1, 3, 2, 2, 3, 1, 2), (64, 1, 6, 2, 2, 5, 0, 1), (32, 2, 6, 2, 2, 2, 0, 2),
            (64, 5, 5, 3, 2, 3, 1, 2), (32, 6, 6, 2, 2, 5, 1, 3), (64, 9, 3, 2, 2, 1, 1, 1), (32, 9, 3, 2, 2, 2, 0, 2),
            (64, 4, 20, 2, 1, 3, 0, 3)]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(tmp_path):
    """every word of inner_product_seeded and of mod_down_add (a separate addend, and the addend exactly out) against
    relin3_exact; the program itself reports a touched guard band"""
    rng = np.random.default_rng(20)
    cases, arrays, want = [], [], []
    for bits, n_power, L, K, alpha, count, off, split in EMULATED:
        M, n, D = L + K, 1 << n_power, -(-L // alpha)
        mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], M)]
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in mods] + mods
        a = random_words(rng, (D, count, M, n), bits, plant)
        key = random_words(rng, (D, 2, M + 1, n), bits, plant)
        c01 = random_words(rng, (2, count, L, n), bits, plant)
        x = random_words(rng, (2 * count, M, n), bits, plant)
        addend = random_words(rng, (2 * count, L, n), bits, plant)
        cases.append((bits, n_power, L, K, alpha, count, off, split, mods))
        arrays.append((a, key, c01, x, addend))
        limbs = [m if m < L else m + 1 for m in range(M)]  # the emulator's plan skips key limb L
        down = exact_mod_down_add(mods[:L], mods[L:], x, addend, bits)
        want.append((exact_seeded(mods, L, a, key, c01, limbs), down, down))
    got, text = run_emulator(tmp_path, emulator_job(cases, arrays))
    assert "vec=0" in text and "vec=1" in text and "rb=4" in text, text
    at = 0
    for case, parts in zip(EMULATED, want):
        for k, w in enumerate(parts):
            part = got[at:at + w.size]
            at += w.size
            assert np.array_equal(from_words(part, w.shape), w), (case, k)
    assert at == got.size
