"""Host side of KeySwitchPlan.multiply_relinearize (include/gpuntt/rns/key_switch.cuh), no GPU: the two kernels' own
text run on CPU threads under the sanitizers, the folded form the kernels compute against the header's three-step
definition in Python integers, and the interface in the built library."""
import ctypes
import os

import numpy as np
import pytest

from hoisted_exact import NARROW, WIDE, host_cases
from innerprod_utils import random_words
from relin_emulator import run_emulator
from relin_exact import exact_definition, exact_multiply_relinearize


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def test_the_kernel_text_on_cpu_threads_under_the_sanitizers(tmp_path):
    """tests/cpp/emulate_relin.cpp: the kern namespace of csrc/relinearize.hip over the digit loop of
    inner_product_internal.hpp, compiled for the HOST (a stand-alone program, one thread per lane) with AddressSanitizer
    and UBSan, against the definitions in exact integers"""
    out = run_emulator(tmp_path)
    assert out.count("tensor_top W=") == 56 and out.count("inner_product_tensor W=") == 56  # 28 cases, u64 and u32
    assert "WRONG" not in out
    for rb in (1, 2, 4):  # every block of inputs, with both loaders
        assert "vec=1 rb=%d" % rb in out and "vec=0 rb=%d" % rb in out


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,L,K,alpha,count", [(1, 3, 2, 2, 1), (3, 3, 2, 2, 2), (5, 3, 2, 2, 3), (4, 6, 2, 2, 1),
                                                      (2, 5, 2, 1, 2)])
def test_the_fold_equals_the_three_step_definition(g, bits, n_power, L, K, alpha, count):
    """P d_c joined to the accumulators before the ModDown gives, word for word, what adding d_c after it gives -- the
    header's argument, here in Python integers alone, on the widest primes and on narrow ones, operands of any words,
    also through key_limbs and for y = x"""
    M, n = L + K, 1 << n_power
    D = -(-L // alpha)
    rng = np.random.default_rng(1000 * bits + 10 * n_power + L)
    for widths in (WIDE[bits], NARROW[bits]):
        cases = host_cases(bits, n_power, widths, M)
        qs = [c.q for c in cases]
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in qs[:L]] + [q for q in qs[:L]]
        x = random_words(rng, (2, count, L, n), bits, plant)
        y = random_words(rng, (2, count, L, n), bits, plant[::-1])
        for km, limbs in ((M, None), (M + 2, list(range(L)) + [L + 2 + k for k in range(K)])):
            key = random_words(rng, (D, 2, km, n), bits, plant)
            for output_ntt in (False, True):
                for other in (y, x):
                    want = exact_definition(cases, L, alpha, bits, x, other, key, output_ntt, limbs)
                    got = exact_multiply_relinearize(cases, L, alpha, bits, x, other, key, output_ntt, limbs)
                    assert got.shape == (2, count, L, n) and np.array_equal(got, want), (widths, km, output_ntt)


def test_the_interface_exists(g):
    lib = ctypes.CDLL(g.LIB_PATH)
    for s in ("u32", "u64"):
        assert hasattr(lib, "gpuntt_keyswitch_plan_multiply_relinearize_" + s)
        assert "gpuntt_keyswitch_plan_multiply_relinearize_" + s in g.EXPORTED_SYMBOLS
    assert callable(g.KeySwitchPlan.multiply_relinearize)
