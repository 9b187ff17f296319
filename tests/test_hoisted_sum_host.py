"""Host side of KeySwitchPlan.rotate_hoisted_sum (include/gpuntt/rns/key_switch.cuh), no GPU: the scratch size, the chunk
rule of inner_product_galois_sum with its read-back, the chunk property seen from the DESTINATION chunk, which is what
that kernel owns, and the kernel's own text run on CPU threads under the sanitizers."""
import os

import numpy as np
import pytest

from hoisted_emulator import run_emulator


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


@pytest.mark.parametrize("bits", [64, 32])
def test_hoisted_sum_scratch_bytes(g, bits):
    """the accumulators T[2][count][M][N] rounded up to 256 bytes as the plan rounds; nothing of it depends on G, so it
    is rotate_hoisted's scratch for one element"""
    word = bits // 8
    f = g.keyswitch_hoisted_sum_scratch_bytes
    for L, K, alpha, n_power in ((6, 2, 2, 12), (3, 2, 2, 5), (1, 1, 1, 1), (20, 2, 1, 9)):
        M = L + K
        for count in (0, 1, 3, 16):
            exact = 2 * count * M * (1 << n_power) * word
            assert f(L, K, alpha, n_power, count, bits) == (exact + 255) // 256 * 256
            assert f(L, K, alpha, n_power, count, bits) == g.keyswitch_hoisted_scratch_bytes(L, K, alpha, n_power, count,
                                                                                              1, bits)
    assert f(1, 1, 1, 1, 1, bits) == 256  # 2 x 1 x 2 x 2 words, rounded up


@pytest.mark.parametrize("bits", [64, 32])
def test_hoisted_sum_scratch_bytes_refuses_arguments_out_of_range(g, bits):
    L, K, alpha, n_power = 6, 2, 2, 12
    for args in ((L, K, alpha, n_power, -1), (L, K, alpha, 0, 1), (L, K, alpha, 29, 1), (0, K, alpha, n_power, 1),
                 (L, 0, alpha, n_power, 1), (60, 5, alpha, n_power, 1), (L, K, 0, n_power, 1)):
        with pytest.raises(ValueError):
            g.keyswitch_hoisted_sum_scratch_bytes(*args, bits)


def test_the_sum_chunk_rule(g):
    """one slot per lane and at most 256 lanes: the largest power of two in [64, 256] with (D + 1) chunk words inside
    32 KiB, at least 64 slots, at most N; LDS within 64 KiB for every D"""
    for bits in (64, 32):
        for D in range(1, 65):
            lc = g.keyswitch_hoist_sum_chunk(bits, D, 28)
            lds = ((D + 1) << lc) * bits // 8
            assert 6 <= lc <= 8 and lds <= 65536
            assert lc == 6 or lds <= 32768
            assert lc == 8 or 2 * lds > 32768
            for n_power in (1, 2, 5, 6, 7):
                assert g.keyswitch_hoist_sum_chunk(bits, D, n_power) == min(lc, n_power)  # capped at N
    assert g.keyswitch_hoist_sum_chunk(64, 3, 16) == 8 and g.keyswitch_hoist_sum_chunk(32, 3, 14) == 8
    assert g.keyswitch_hoist_sum_chunk(64, 20, 9) == 7 and g.keyswitch_hoist_sum_chunk(32, 20, 9) == 8
    assert g.keyswitch_hoist_sum_chunk(64, 64, 16) == 6
    for bad in ((16, 3, 12), (64, 0, 12), (64, 65, 12), (64, 3, 0), (64, 3, 29)):
        with pytest.raises(ValueError):
            g.keyswitch_hoist_sum_chunk(*bad)


def test_the_chunk_hook_forces_the_sum_chunk_too_and_restores(g):
    auto = {(bits, D): g.keyswitch_hoist_sum_chunk(bits, D, 16) for bits in (64, 32) for D in (1, 3, 20, 64)}
    try:
        for lc in (6, 7, 8):
            g.set_test_hook("keyswitch_hoist_chunk", lc)
            assert g.keyswitch_hoist_sum_chunk(64, 3, 16) == lc and g.keyswitch_hoist_sum_chunk(64, 3, 5) == 5
        for lc in (9, 11, 13):  # beyond one slot per lane of 256: capped there
            g.set_test_hook("keyswitch_hoist_chunk", lc)
            assert g.keyswitch_hoist_sum_chunk(32, 1, 16) == 8 and g.keyswitch_hoist_sum_chunk(64, 3, 5) == 5
    finally:
        g.set_test_hook("keyswitch_hoist_chunk", 0)
    assert auto == {(bits, D): g.keyswitch_hoist_sum_chunk(bits, D, 16) for bits in (64, 32) for D in (1, 3, 20, 64)}


def test_a_forced_sum_chunk_still_fits_a_workgroup(g):
    try:
        g.set_test_hook("keyswitch_hoist_chunk", 13)
        for bits in (64, 32):
            for D in range(1, 65):
                lc = g.keyswitch_hoist_sum_chunk(bits, D, 16)
                assert 6 <= lc <= 8 and ((D + 1) << lc) * bits // 8 <= 65536
        assert g.keyswitch_hoist_sum_chunk(64, 64, 16) == 6 and g.keyswitch_hoist_sum_chunk(64, 31, 16) == 8
        assert g.keyswitch_hoist_sum_chunk(64, 32, 16) == 7
    finally:
        g.set_test_hook("keyswitch_hoist_chunk", 0)


def test_the_rotation_chunk_read_back_is_what_it_was(g):
    """the values tests/test_hoisted_rotation_host.py pins for inner_product_galois, with and without the hook"""
    assert g.keyswitch_hoist_chunk(64, 64, 28) == 6 and g.keyswitch_hoist_chunk(64, 3, 28) == 10
    assert g.keyswitch_hoist_chunk(32, 3, 28) == 11 and g.keyswitch_hoist_chunk(64, 3, 5) == 5
    assert g.keyswitch_hoist_chunk(64, 20, 9) == 7 and g.keyswitch_hoist_chunk(32, 20, 9) == 8
    try:
        for lc in (6, 9, 11):
            g.set_test_hook("keyswitch_hoist_chunk", lc)
            assert g.keyswitch_hoist_chunk(64, 3, 16) == lc and g.keyswitch_hoist_chunk(64, 3, 5) == 5
        g.set_test_hook("keyswitch_hoist_chunk", 13)
        assert g.keyswitch_hoist_chunk(32, 1, 16) == 13 and g.keyswitch_hoist_chunk(64, 3, 16) == 11
        assert g.keyswitch_hoist_chunk(64, 64, 16) == 6
    finally:
        g.set_test_hook("keyswitch_hoist_chunk", 0)
    assert g.keyswitch_hoist_chunk(64, 3, 28) == 10


def hoisted_elements(g, n_power, G=8):
    """the elements of tests/test_gpu_hoisted_sum.py (hoisted_utils.elements_for, restated: that module needs the oracle
    build)"""
    base = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_rotation(-1, n_power),
            g.galois_element_for_conjugation(n_power), 1]
    return base + [g.galois_element_for_rotation(s, n_power) for s in range(2, G)]


@pytest.mark.parametrize("poly", ["plus", "minus"])
def test_every_destination_chunk_has_one_source_chunk_per_element(g, poly):
    """what inner_product_galois_sum relies on, at every chunk it can choose (64, 128, 256 slots): the source chunk of a
    destination chunk is the source chunk of its FIRST slot, and the low 6 slot bits stay within 64 consecutive source
    words (a wave reads a permutation of 64 consecutive LDS words)"""
    reduction = g.X_N_plus if poly == "plus" else g.X_N_minus
    n_power = 11
    n = 1 << n_power
    for k in hoisted_elements(g, n_power):
        src = g.automorphism_index_map(n_power, k, reduction).astype(np.int64)
        assert np.array_equal(np.sort(src), np.arange(n))
        for c in (6, 7, 8):
            chunks = (src >> c).reshape(n >> c, 1 << c)
            assert (chunks == chunks[:, :1]).all(), (k, c)
            assert np.array_equal(np.sort(chunks[:, 0]), np.arange(n >> c))
        low = (src >> 6).reshape(-1, 64)
        assert (low == low[:, :1]).all(), k
        assert np.array_equal(np.sort((src & 63).reshape(-1, 64), axis=1), np.broadcast_to(np.arange(64), low.shape))


def test_the_kernel_text_on_cpu_threads_under_the_sanitizers(tmp_path):
    """tests/cpp/emulate_hoisted.cpp sum: the kern namespace of csrc/hoisted_rotation.hip compiled for the HOST (a
    stand-alone program, one thread per lane) with AddressSanitizer and UBSan, against the definition in exact integers"""
    out = run_emulator(tmp_path, "sum")
    assert out.count("sum W=") == 34 and "rotation W=" not in out  # 17 cases, u64 and u32
