"""Host side of KeySwitchPlan.multiply_relinearize_sum (include/gpuntt/rns/key_switch.cuh), no GPU: the two kernels' own
text run on CPU threads under the sanitizers, the folded form the kernels compute against the header's three-step
definition in Python integers, and the interface in the built library."""
import ctypes
import os

import numpy as np
import pytest

from hoisted_exact import NARROW, WIDE, host_cases
from innerprod_utils import random_words
from relin_exact import exact_definition
from relin_sum_emulator import run_sum_emulator
from relin_sum_exact import exact_multiply_relinearize_sum, exact_sum_definition


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def test_the_kernel_text_on_cpu_threads_under_the_sanitizers(tmp_path):
    """tests/cpp/emulate_relin_sum.cpp: the kern namespace of csrc/relinearize_sum.hip over the digit loop of
    inner_product_internal.hpp, compiled for the HOST (a stand-alone program, one thread per lane) with AddressSanitizer
    and UBSan, against the definitions in exact integers"""
    out = run_sum_emulator(tmp_path)
    cases = 37  # u64 and u32 each
    assert out.count("tensor_top_sum W=") == 2 * cases and out.count("inner_product_tensor_sum W=") == 2 * cases
    assert "WRONG" not in out
    for rb in (1, 2):  # every block of inputs, with both loaders
        assert "vec=1 rb=%d" % rb in out and "vec=0 rb=%d" % rb in out
    for terms in (1, 2, 3, 32):
        assert " terms=%d " % terms in out
    # one operand of one term one word off alignment switches the whole case to the one-word loader
    lines = [ln for ln in out.splitlines() if " one_off=1 " in ln]
    assert len(lines) == 12 and all(" vec=0 " in ln for ln in lines)
    assert any(" ones=1 " in ln and " terms=32 " in ln for ln in out.splitlines())  # the largest carry count
    assert " same=1 " in out and " dup=1 " in out


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,L,K,alpha,count,terms", [(1, 3, 2, 2, 1, 1), (3, 3, 2, 2, 2, 2), (4, 3, 2, 2, 3, 5),
                                                            (3, 6, 2, 2, 1, 2), (2, 5, 2, 1, 2, 5)])
def test_the_fold_equals_the_three_step_definition(g, bits, n_power, L, K, alpha, count, terms):
    """P d_c joined to the accumulators before the ModDown gives, word for word, what adding d_c after it gives, d_c
    being the sums over the terms -- in Python integers alone, on the widest primes and on narrow ones, operands of any
    words, through key_limbs, with a squared term and a tensor used in two terms; with one term it is
    multiply_relinearize's definition"""
    M, n = L + K, 1 << n_power
    D = -(-L // alpha)
    rng = np.random.default_rng(1000 * bits + 10 * n_power + L + terms)
    for widths in (WIDE[bits], NARROW[bits]):
        cases = host_cases(bits, n_power, widths, M)
        qs = [c.q for c in cases]
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in qs[:L]] + [q for q in qs[:L]]
        xs = [random_words(rng, (2, count, L, n), bits, plant) for _ in range(terms)]
        ys = [random_words(rng, (2, count, L, n), bits, plant[::-1]) for _ in range(terms)]
        ys[-1] = xs[-1]  # a squared term
        if terms > 2:
            xs[1] = xs[0]  # one tensor in two terms
        for km, limbs in ((M, None), (M + 2, list(range(L)) + [L + 2 + k for k in range(K)])):
            key = random_words(rng, (D, 2, km, n), bits, plant)
            for output_ntt in (False, True):
                want = exact_sum_definition(cases, L, alpha, bits, xs, ys, key, output_ntt, limbs)
                got = exact_multiply_relinearize_sum(cases, L, alpha, bits, xs, ys, key, output_ntt, limbs)
                assert got.shape == (2, count, L, n) and np.array_equal(got, want), (widths, km, output_ntt)
                if terms == 1:
                    one = exact_definition(cases, L, alpha, bits, xs[0], ys[0], key, output_ntt, limbs)
                    assert np.array_equal(got, one), (widths, km, output_ntt)


def test_the_interface_exists(g):
    lib = ctypes.CDLL(g.LIB_PATH)
    for s in ("u32", "u64"):
        assert hasattr(lib, "gpuntt_keyswitch_plan_multiply_relinearize_sum_" + s)
        assert "gpuntt_keyswitch_plan_multiply_relinearize_sum_" + s in g.EXPORTED_SYMBOLS
    assert callable(g.KeySwitchPlan.multiply_relinearize_sum)


def test_the_wrapper_refuses_bad_lists_before_it_loads_anything(pkg, monkeypatch):
    """an empty list and lists of unequal length: ValueError before the library is touched"""
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(pkg, "load_library", no_library)
    plan = object.__new__(pkg.KeySwitchPlan)  # no handle: the refusals need none
    with pytest.raises(ValueError):
        plan.multiply_relinearize_sum([], [], None, None, 1, True, None)
    with pytest.raises(ValueError):
        plan.multiply_relinearize_sum([object()], [object(), object()], None, None, 1, True, None)
    with pytest.raises(ValueError):
        plan.multiply_relinearize_sum([object()], [], None, None, 1, True, None)
