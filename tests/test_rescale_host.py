"""Host side of KeySwitchPlan's rescaling calls (include/gpuntt/rns/key_switch.cuh, "Rescaling"), no GPU: the two host
references against Python integers, the folded form against the header's definition and against the two-step result, the
kernels' own text on CPU threads under the sanitizers, the refusals that need no device and the interface of the built
library.  Every comparison is array_equal."""
import ctypes
import os

import numpy as np
import pytest

from hoisted_exact import NARROW, WIDE, host_cases
from innerprod_utils import from_words, random_words, words
from relin_exact import exact_multiply_relinearize
from rescale_exact import (centred_difference, exact_definition_rescale, exact_multiply_relinearize_rescale,
                           folded_stack, in_band, ref_mod_down_rescale, ref_rescale)
from rescale_utils import run_emulator

# (L, K, R): the last two leave ONE kept limb, R = L - 1
SHAPES = [(3, 2, 1), (6, 2, 2), (4, 1, 3), (2, 1, 1)]


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def planted(rng, shape, bits, qs):
    top = (1 << bits) - 1
    x = random_words(rng, shape, bits, [0, top] + [q - 1 for q in qs] + [q for q in qs])
    for i, q in enumerate(qs):  # every limb sees its own extremes
        x[0, i, 0], x[-1, i, -1] = q - 1, top
        x[0, i, -1], x[-1, i, 0] = q, 0
    return x


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5])
@pytest.mark.parametrize("stacks", [1, 3])
@pytest.mark.parametrize("L,K,R", SHAPES)
def test_the_references_equal_python_integers(g, bits, n_power, stacks, L, K, R):
    """reference_mod_down_rescale and reference_rescale (unsigned __int128 and %) against rescale_exact, which restates
    the split {dropped q, p} -> {kept q} and converts with keyswitch_utils.ref_convert; the widest primes and narrow ones;
    0, 2^W - 1, q - 1 and q planted in every limb"""
    M, n = L + K, 1 << n_power
    rng = np.random.default_rng(bits + 10 * n_power + 100 * stacks + 1000 * L)
    for widths in (WIDE[bits], NARROW[bits]):
        moduli = [c.q for c in host_cases(bits, n_power, widths, M)]
        qs, ps = moduli[:L], moduli[L:]
        x = planted(rng, (stacks, M, n), bits, moduli)
        out = np.zeros(stacks * (L - R) * n, dtype=g.np_dtype(bits))
        g.keyswitch_reference_mod_down_rescale(qs, ps, R, words(g, x, bits), out, n_power, stacks, bits=bits)
        want = ref_mod_down_rescale(qs, ps, R, x, bits)
        assert np.array_equal(from_words(out, want.shape), want), widths
        xq = planted(rng, (stacks, L, n), bits, qs)
        out = np.zeros(stacks * (L - R) * n, dtype=g.np_dtype(bits))
        g.keyswitch_reference_rescale(qs, R, words(g, xq, bits), out, n_power, stacks, bits=bits)
        want = ref_rescale(qs, R, xq, bits)
        assert np.array_equal(from_words(out, want.shape), want), widths


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,L,K,alpha,R,count", [(1, 3, 2, 2, 1, 1), (3, 6, 2, 2, 2, 2), (5, 3, 2, 2, 1, 3),
                                                        (4, 4, 1, 2, 3, 1), (2, 2, 1, 1, 1, 2)])
def test_the_fold_equals_the_definition_and_stays_within_one_of_two_steps(g, bits, n_power, L, K, alpha, R, count):
    """In Python integers alone.  (1) P d_c joined to the accumulators in the NTT domain, before the inverse transform,
    gives word for word what the header's definition of multiply_relinearize_rescale gives (P d_c added to the q-limbs of
    the coefficient-form stack).  (2) The fused result, round(X / (P Q_R)), differs from the two-step result
    round(round(X / P) / Q_R) -- multiply_relinearize, then rescale -- by at most 1, centred modulo the kept base, at
    every coefficient where none of the three conversions lies in its rounding band; band membership is computed exactly
    and at most 0.1 % of the coefficients may be skipped for it."""
    M, n = L + K, 1 << n_power
    rng = np.random.default_rng(77 * bits + 10 * n_power + L)
    skipped = total = 0
    for widths in (WIDE[bits], NARROW[bits]):
        cases = host_cases(bits, n_power, widths, M)
        qs = [c.q for c in cases]
        D = -(-L // alpha)
        top = (1 << bits) - 1
        plant = [0, top] + [q - 1 for q in qs[:L]] + [q for q in qs[:L]]
        x = random_words(rng, (2, count, L, n), bits, plant)
        y = random_words(rng, (2, count, L, n), bits, plant[::-1])
        key = random_words(rng, (D, 2, M, n), bits, plant)
        for other in (y, x):
            for output_ntt in (False, True):
                want = exact_definition_rescale(cases, L, R, alpha, bits, x, other, key, output_ntt)
                got = exact_multiply_relinearize_rescale(cases, L, R, alpha, bits, x, other, key, output_ntt)
                assert got.shape == (2, count, L - R, n) and np.array_equal(got, want), (widths, output_ntt)
            fused = exact_multiply_relinearize_rescale(cases, L, R, alpha, bits, x, other, key, False)
            one = exact_multiply_relinearize(cases, L, alpha, bits, x, other, key, False)  # [2][count][L][N]
            two = ref_rescale(qs[:L], R, one.reshape(2 * count, L, n), bits).reshape(fused.shape)
            stack = folded_stack(cases, L, alpha, bits, x, other, key).reshape(2 * count, M, n)
            band = in_band(qs[L:], np.moveaxis(stack[:, L:, :], 1, 0), bits)           # mod_down: the base p
            band |= in_band(qs[L - R:], np.moveaxis(stack[:, L - R:, :], 1, 0), bits)   # mod_down_rescale
            band |= in_band(qs[L - R:L], np.moveaxis(one.reshape(2 * count, L, n)[:, L - R:, :], 1, 0), bits)  # rescale
            diff = centred_difference(qs[:L - R], fused, two).reshape(2 * count, n)
            clear = ~band
            assert all(abs(int(v)) <= 1 for v in diff[clear]), (widths, max(abs(int(v)) for v in diff[clear]))
            skipped, total = skipped + int(band.sum()), total + band.size
    assert skipped * 1000 <= total, (skipped, total)


def test_the_kernel_text_on_cpu_threads_under_the_sanitizers(tmp_path):
    """tests/cpp/emulate_rescale.cpp: the kern namespace of csrc/rescale.hip compiled for the HOST (a stand-alone program,
    one thread per lane) with AddressSanitizer and UBSan, against exact integers: both widths, both loaders, N = 2 .. 512,
    pointers one word off alignment, every operand word 2^W - 1, moduli within an eighth below 2^(W-2)"""
    out = run_emulator(tmp_path)
    assert out.count("rescale_gather W=") == 46 and out.count("rescale_sub_scale W=") == 46  # 23 cases, u64 and u32
    assert "WRONG" not in out
    for w in (64, 32):
        assert "rescale_sub_scale W=%d n=1 " % w in out and "rescale_sub_scale W=%d n=9 " % w in out
        for vec in (0, 1):
            assert any(l.startswith("rescale_sub_scale W=%d" % w) and l.rstrip().endswith("vec=%d: ok (0)" % vec)
                       for l in out.splitlines()), (w, vec)
    assert "W=32 n=1 L=3 R=1 stacks=1 off=0 top=0 ones=0 vec=0" in out  # N = 2 at u32: below a 16-byte group
    assert "off=1 top=1 ones=1" in out


@pytest.mark.parametrize("bits", [64, 32])
def test_refusals_without_a_device(g, bits):
    n_power, L, K = 3, 3, 2
    n = 1 << n_power
    moduli = [c.q for c in host_cases(bits, n_power, NARROW[bits], L + K)]
    qs, ps = moduli[:L], moduli[L:]
    dt = g.np_dtype(bits)
    x, xq, out = np.zeros(2 * (L + K) * n, dtype=dt), np.zeros(2 * L * n, dtype=dt), np.zeros(2 * L * n, dtype=dt)
    for R in (-1, 0, L, L + 1):  # the references take R in [1, L - 1]: R = 0 is a plan without rescale_limbs
        with pytest.raises(ValueError, match="Invalid rescale_limbs!"):
            g.keyswitch_reference_mod_down_rescale(qs, ps, R, x, out, n_power, 2, bits=bits)
        with pytest.raises(ValueError, match="Invalid rescale_limbs!"):
            g.keyswitch_reference_rescale(qs, R, xq, out, n_power, 2, bits=bits)
    for R in (-1, L, L + 1):  # workspace_bytes and the constructor take R in [0, L - 1]
        with pytest.raises(ValueError, match="Invalid rescale_limbs!"):
            g.KeySwitchPlan.workspace_bytes(L, K, 2, n_power, bits, rescale_limbs=R)
    bad = [lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, None, out, n_power, 2, bits=bits),
           lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, None, n_power, 2, bits=bits),
           lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, out, n_power, -1, bits=bits),
           lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, out, 0, 2, bits=bits),
           lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, x[n:], n_power, 2, bits=bits),   # an overlap
           lambda: g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, x, n_power, 2, bits=bits),       # in place
           lambda: g.keyswitch_reference_mod_down_rescale(qs, [qs[0]], 1, x, out, n_power, 2, bits=bits),  # not coprime
           lambda: g.keyswitch_reference_rescale(qs, 1, None, out, n_power, 2, bits=bits),
           lambda: g.keyswitch_reference_rescale(qs, 1, xq, None, n_power, 2, bits=bits),
           lambda: g.keyswitch_reference_rescale(qs, 1, xq, out, n_power, -1, bits=bits),
           lambda: g.keyswitch_reference_rescale(qs, 1, xq, out, 29, 2, bits=bits),
           lambda: g.keyswitch_reference_rescale(qs, 1, xq, xq[n:], n_power, 2, bits=bits),              # an overlap
           lambda: g.keyswitch_reference_rescale(qs, 1, xq, xq, n_power, 2, bits=bits),                  # in place
           lambda: g.keyswitch_reference_rescale([qs[0], qs[1], qs[0]], 1, xq, out, n_power, 2, bits=bits),
           lambda: g.keyswitch_reference_rescale([qs[0], qs[0], qs[1]], 1, xq, out, n_power, 2, bits=bits)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    # stacks = 0 is not an error and writes nothing
    keep = out.copy()
    g.keyswitch_reference_rescale(qs, 1, xq, out, n_power, 0, bits=bits)
    g.keyswitch_reference_mod_down_rescale(qs, ps, 1, x, out, n_power, 0, bits=bits)
    assert np.array_equal(out, keep)


def test_the_interface_exists_and_R_zero_is_the_old_workspace(g):
    lib = ctypes.CDLL(g.LIB_PATH)
    names = ("plan_workspace_bytes_rescale", "plan_create_rescale", "plan_rescale_limbs", "plan_rescale_scratch_bytes",
             "plan_mod_down_rescale", "plan_rescale", "plan_multiply_relinearize_rescale",
             "plan_multiply_relinearize_sum_rescale", "plan_rotate_hoisted_sum_rescale", "reference_mod_down_rescale",
             "reference_rescale")
    for s in ("u32", "u64"):
        for name in names:
            assert hasattr(lib, "gpuntt_keyswitch_%s_%s" % (name, s)), name
            assert "gpuntt_keyswitch_%s_%s" % (name, s) in g.EXPORTED_SYMBOLS, name
    for name in ("mod_down_rescale", "rescale", "rescale_scratch_bytes", "multiply_relinearize_rescale",
                 "multiply_relinearize_sum_rescale", "rotate_hoisted_sum_rescale"):
        assert callable(getattr(g.KeySwitchPlan, name)), name
    assert isinstance(g.KeySwitchPlan.rescale_limbs, property)
    assert callable(g.keyswitch_reference_mod_down_rescale) and callable(g.keyswitch_reference_rescale)
    for bits in (64, 32):
        for L, K, alpha, n_power in ((3, 2, 2, 5), (6, 2, 2, 12), (4, 1, 2, 16), (2, 1, 1, 1), (40, 24, 20, 9)):
            old = g.KeySwitchPlan.workspace_bytes(L, K, alpha, n_power, bits)
            assert g.KeySwitchPlan.workspace_bytes(L, K, alpha, n_power, bits, rescale_limbs=0) == old
            got = ctypes.c_uint64()  # R = 0 through the new symbol itself
            fn = getattr(lib, "gpuntt_keyswitch_plan_workspace_bytes_rescale_u%d" % bits)
            assert fn(L, K, alpha, n_power, 0, ctypes.byref(got)) == 0 and got.value == old
            for R in (1, L - 1):
                assert g.KeySwitchPlan.workspace_bytes(L, K, alpha, n_power, bits, rescale_limbs=R) > old
