"""Host side of KeySwitchPlan.rotate_hoisted (include/gpuntt/rns/key_switch.cuh), no GPU: the scratch size, the identity
that lets the kernel fold c0 in before the ModDown, the chunk property at every chunk size the kernel can choose, and the
kernel's own text run on CPU threads under the sanitizers."""
import math
import os

import numpy as np
import pytest

from innerprod_utils import from_words, moduli, random_words, words
from hoisted_emulator import run_emulator
from keyswitch_utils import ref_mod_down


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


@pytest.mark.parametrize("bits", [64, 32])
def test_hoisted_scratch_bytes(g, bits):
    """at least the accumulators T[G][2][count][M][N], monotone in G and count, out-of-range arguments refused"""
    L, K, alpha, n_power = 6, 2, 2, 12
    M, word = L + K, bits // 8
    f = g.keyswitch_hoisted_scratch_bytes
    for G in (1, 2, 5, 64):
        for count in (0, 1, 3, 16):
            b = f(L, K, alpha, n_power, count, G, bits)
            assert b >= G * 2 * count * M * (1 << n_power) * word and b % 256 == 0
            if G < 64:
                assert f(L, K, alpha, n_power, count, G + 1, bits) >= b
            assert f(L, K, alpha, n_power, count + 1, G, bits) >= b
    assert f(1, 1, 1, 1, 1, 1, bits) >= 2 * 2 * 2 * word
    for args in ((L, K, alpha, n_power, 1, 0), (L, K, alpha, n_power, 1, 65), (L, K, alpha, n_power, 1, -1),
                 (L, K, alpha, n_power, -1, 1), (L, K, alpha, 0, 1, 1), (L, K, alpha, 29, 1, 1),
                 (0, K, alpha, n_power, 1, 1), (L, 0, alpha, n_power, 1, 1), (60, 5, alpha, n_power, 1, 1),
                 (L, K, 0, n_power, 1, 1)):
        with pytest.raises(ValueError):
            f(*args, bits)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K", [(1, 1), (5, 2), (3, 3)])
def test_folding_p_times_y_in_before_the_mod_down_is_exact(g, bits, L, K):
    """mod_down(x + P y on the q-limbs) == (y + mod_down(x)) mod q, limb for limb: the special limbs are untouched, so
    the conversion term is the same, and (c + P y - conv) P^-1 = y + (c - conv) P^-1 (mod q).  In Python integers
    (keyswitch_utils.ref_mod_down) and through the library's host reference."""
    ms = moduli(bits, L + K)
    qs, ps = ms[:L], ms[L:]
    P, M, n_power, stacks = math.prod(ps), L + K, 4, 3
    n = 1 << n_power
    rng = np.random.default_rng(10 * L + K + bits)
    x = np.stack([random_words(rng, (stacks, n), bits) % q for q in ms], axis=1)      # [stacks][M][N], canonical
    y = np.stack([random_words(rng, (stacks, n), bits) % q for q in qs], axis=1)      # [stacks][L][N]
    x[0, :, 0] = [q - 1 for q in ms]  # extremes: the largest residues everywhere, and zeros
    y[0, :, 0] = [q - 1 for q in qs]
    x[1, :, 1], y[1, :, 1] = 0, 0
    folded = x.copy()
    for j, q in enumerate(qs):
        folded[:, j, :] = (x[:, j, :] + P * y[:, j, :]) % q
    qcol = np.array(qs, dtype=object)[None, :, None]
    want = (y + ref_mod_down(qs, ps, x, bits)) % qcol
    assert np.array_equal(ref_mod_down(qs, ps, folded, bits), want)

    def library(v):
        out = np.zeros(stacks * L * n, dtype=g.np_dtype(bits))
        g.keyswitch_reference_mod_down(qs, ps, words(g, v, bits), out, n_power, stacks, bits)
        return from_words(out, (stacks, L, n))

    assert np.array_equal(library(x), ref_mod_down(qs, ps, x, bits))
    assert np.array_equal(library(folded), want)


def hoisted_elements(g, n_power, G=8):
    """the elements of tests/test_gpu_hoisted_rotation.py (hoisted_utils.elements_for, restated: that module needs the
    oracle build)"""
    base = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_rotation(-1, n_power),
            g.galois_element_for_conjugation(n_power), 1]
    return base + [g.galois_element_for_rotation(s, n_power) for s in range(2, G)]


@pytest.mark.parametrize("poly", ["plus", "minus"])
def test_chunk_property_at_every_chunk_the_kernel_can_choose(g, poly):
    """every destination chunk of 2^c slots is filled from exactly one source chunk, for c = 6 .. the automatic chunk
    of the shapes the GPU tests run (and the largest the rule can give: D = 1, 32-bit words)"""
    reduction = g.X_N_plus if poly == "plus" else g.X_N_minus
    n_power = 13
    n = 1 << n_power
    auto = {(bits, D): g.keyswitch_hoist_chunk(bits, D, 28) for bits in (64, 32) for D in (1, 2, 3, 20, 64)}
    # the budget rule: the largest power of two with (D + 1) chunk words inside 32 KiB, at least 64 slots
    for (bits, D), lc in auto.items():
        assert lc >= 6 and (lc == 6 or ((D + 1) << lc) * bits // 8 <= 32768) and ((D + 1) << (lc + 1)) * bits // 8 > 32768
    assert auto[(64, 64)] == 6 and auto[(64, 3)] == 10 and auto[(32, 3)] == 11
    assert g.keyswitch_hoist_chunk(64, 3, 5) == 5  # capped at N
    top = max(auto.values())
    assert top <= n_power
    for k in hoisted_elements(g, n_power):
        src = g.automorphism_index_map(n_power, k, reduction).astype(np.int64)
        assert np.array_equal(np.sort(src), np.arange(n))
        for c in range(6, top + 1):
            chunks = (src >> c).reshape(n >> c, 1 << c)
            assert (chunks == chunks[:, :1]).all(), (k, c)  # one source chunk per destination chunk
            assert np.array_equal(np.sort(chunks[:, 0]), np.arange(n >> c))  # and every source chunk lands somewhere
            # the low 6 slot bits permute within 64 consecutive words (what makes the LDS read conflict-free)
            low = (src & 63).reshape(-1, 64)
            assert np.array_equal(np.sort(low, axis=1), np.broadcast_to(np.arange(64), low.shape))


def test_the_chunk_hook_is_read_back(g):
    try:
        for lc in (6, 9, 11):
            g.set_test_hook("keyswitch_hoist_chunk", lc)
            assert g.keyswitch_hoist_chunk(64, 3, 16) == lc and g.keyswitch_hoist_chunk(64, 3, 5) == 5
        g.set_test_hook("keyswitch_hoist_chunk", 13)  # a forced chunk still has to fit the 64 KiB of a workgroup
        assert g.keyswitch_hoist_chunk(32, 1, 16) == 13 and g.keyswitch_hoist_chunk(64, 3, 16) == 11
        assert g.keyswitch_hoist_chunk(64, 64, 16) == 6
        for bad in (1, 5, 14, -1):
            with pytest.raises(ValueError):
                g.set_test_hook("keyswitch_hoist_chunk", bad)
    finally:
        g.set_test_hook("keyswitch_hoist_chunk", 0)


def test_the_kernel_text_on_cpu_threads_under_the_sanitizers(tmp_path):
    """tests/cpp/emulate_hoisted.cpp rotation: the kern namespace of csrc/hoisted_rotation.hip compiled for the HOST (a
    stand-alone program, one thread per lane) with AddressSanitizer and UBSan, against the definition in exact integers,
    with moduli below 2^(W-3) and just below 2^(W-2) and with every operand word 2^W - 1 at 64 elements and 64 digits"""
    out = run_emulator(tmp_path, "rotation")
    assert out.count("rotation W=") == 40 and "sum W=" not in out  # 10 cases, two widths of the moduli, u64 and u32
