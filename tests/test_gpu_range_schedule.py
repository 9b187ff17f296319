"""-m gpu: forward 64-bit Merge transforms through the C ABI against the CPU oracle, every word, at the shapes and moduli
where the whole-pass range plans (csrc/lazy.hpp: ct_sched; a quotient estimate in mid-pass, hand-off caps between the
two passes of the rings 2^14 and 2^16) choose the kernels:

    ring 2^16  batch 4   four-polynomial tile of the 10-stage last pass
    ring 2^16  batch 3   one-polynomial tile
    ring 2^14  batch 4   strided pass of 4 stages with a capped hand-off + the 10-stage last pass
    ring 2^15  batch 4   7 strided + 8 contiguous stages: planned pass by pass, uncapped hand-off
    ring 2^12  batch 2   single pass
    ring 2^17  batch 2   6 strided + 11 contiguous stages, uncapped hand-off
    ring 2^16, stack of two primes, batch 8
    rings 2^16 and 2^14, batch 4, X^N - 1: the unit-twiddle first stage of the capped strided kernels

with the pool prime of the ring, the largest prime = 1 (mod 2^17) with 31 q < 2^64, a 60-bit prime (16 q range), a 61-bit
prime (8 q range: no whole-pass plan) and a 45-bit prime (the quotient estimate shifts the word).  Inputs: random
residues, q - 1 everywhere, zero everywhere, 0 / q - 1 alternating at stride 1 and at stride N / 2.  In place and out of
place; GPU_INTT of the result gives the input back.  Random words do not reach the range edges -- those are proved by
tests/test_range_schedule_host.py; this file checks that the planned kernels compute the transform."""
import os

import numpy as np
import pytest

from gpu_utils import MergeCase, _is_probable_prime, find_ntt_factors, oracle_batch, rns_stack
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4), (16, 3), (14, 4), (15, 4), (12, 2), (17, 2)]
MODULI = ["pool", "top31", "b60", "b61", "b45"]
FAMILY = {"pool": 31, "top31": 31, "b60": 0, "b61": 8, "b45": 31}
PATTERNS = ["random", "qm1", "zero", "alt1", "althalf"]


@pytest.fixture(scope="module")
def g(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def top31_factors(logn):
    """(q, omega, psi): the largest prime = 1 (mod 2^max(17, logn + 1)) not above floor((2^64 - 1) / 31)"""
    step = 1 << max(17, logn + 1)
    q = ((1 << 64) - 1) // 31 // step * step + 1
    while q > ((1 << 64) - 1) // 31 or not _is_probable_prime(q):
        q -= step
    gen = 2
    while True:
        psi = pow(gen, (q - 1) >> (logn + 1), q)
        if pow(psi, 1 << logn, q) == q - 1:
            return q, psi * psi % q, psi
        gen += 1


def factors_of(modulus, logn):
    if modulus == "pool":
        return None
    if modulus == "top31":
        return top31_factors(logn)
    return find_ntt_factors(int(modulus[1:]), logn, clear_of_top=True)


def pattern(c, name, batch, seed):
    n, q = c.n, c.q
    i = np.arange(batch * n) % n
    if name == "random":
        return c.random(batch, seed)
    if name == "qm1":
        return np.full(batch * n, q - 1, dtype=c.P.T)
    if name == "zero":
        return np.zeros(batch * n, dtype=c.P.T)
    if name == "alt1":
        return np.where(i % 2 == 1, q - 1, 0).astype(c.P.T)
    return np.where(i >= n // 2, q - 1, 0).astype(c.P.T)


_cases = {}


def case_of(g, modulus, logn, poly=O.X_N_plus):
    key = (modulus, logn, poly)
    if key not in _cases:
        _cases[key] = MergeCase(g, 64, logn, poly, factors_of(modulus, logn))
    return _cases[key]


def test_the_moduli_sit_in_the_families_they_are_meant_for():
    top = ((1 << 64) - 1) // 31
    q = top31_factors(16)[0]
    assert q <= top and q % (1 << 17) == 1 and 31 * q < (1 << 64)
    assert not any(_is_probable_prime(p) for p in range(q + (1 << 17), top + 1, 1 << 17))
    assert find_ntt_factors(45, 16, clear_of_top=True)[0].bit_length() == 45
    assert find_ntt_factors(60, 16, clear_of_top=True)[0] > top  # 16 q range, not 31 q
    assert find_ntt_factors(61, 16, clear_of_top=True)[0].bit_length() == 61


@pytest.mark.parametrize("modulus", ["pool", "b60"])
@pytest.mark.parametrize("logn", [16, 14])
def test_cyclic_forward_matches_the_oracle_and_round_trips(g, logn, modulus):
    """X^N - 1 (the flagship's polynomial): the first stage of the capped strided pass takes its twiddle-is-one path"""
    check_shape(g, case_of(g, modulus, logn, O.X_N_minus), modulus, logn, 4)


@pytest.mark.parametrize("modulus", MODULI)
@pytest.mark.parametrize("logn,batch", SHAPES)
def test_forward_matches_the_oracle_and_round_trips(g, logn, batch, modulus):
    check_shape(g, case_of(g, modulus, logn), modulus, logn, batch)


def check_shape(g, c, modulus, logn, batch):
    fam = "merge_pass_lazy:%d" % FAMILY[modulus]
    for k, name in enumerate(PATTERNS):
        x = pattern(c, name, batch, 0x5C4ED + 16 * logn + k)
        want = oracle_batch([c], x)
        for inplace in (True, False):
            with g.launch_log() as log:
                got = c.gpu_forward(np.array(x), inplace=inplace)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s 2^%d x %d %s inplace=%s: %d words differ, first at %d" % (
                modulus, logn, batch, name, inplace, bad.size, bad[0])
            assert fam in log.kernels, log.kernels
            back = c.gpu_inverse(got, inplace=inplace)
            assert np.array_equal(back, x), "%s 2^%d x %d %s inplace=%s: no round trip" % (modulus, logn, batch, name, inplace)


@pytest.mark.parametrize("widths,family", [((59, 58), 31), ((60, 60), 0)])
def test_rns_stack_of_two_primes_2_16_batch_8(g, widths, family):
    import torch
    logn, batch, poly = 16, 8, O.X_N_plus
    n = 1 << logn
    cases, fwd, inv = rns_stack(g, 64, logn, list(widths), poly)
    mc = len(cases)
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], 64)
    cfg = g.ntt_rns_configuration(n_power=logn, reduction_poly=poly)

    def forward(x, inplace):
        d = g.to_device(x)
        out = d if inplace else torch.zeros_like(d)
        if inplace:
            g.GPU_NTT_Inplace(d, fwd, mods, cfg, batch, mc)
        else:
            g.GPU_NTT(d, out, fwd, mods, cfg, batch, mc)
        torch.cuda.synchronize()
        return g.to_host(out)

    g.set_test_hook("reset_predictions", "1")  # whatever stack lived at this address before
    forward(np.concatenate([cases[p % mc].random(1, 3 + p) for p in range(batch)]), False)  # the family prediction settles
    fam = "merge_pass_lazy:%d" % family
    for k, name in enumerate(PATTERNS):
        x = np.concatenate([pattern(cases[p % mc], name, 1, 0xA11 + 8 * k + p) for p in range(batch)])
        want = oracle_batch(cases, x)
        for inplace in (True, False):
            with g.launch_log() as log:
                got = forward(np.array(x), inplace)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s %s inplace=%s: %d words differ, first at %d" % (widths, name, inplace, bad.size, bad[0])
            assert log.kernels.count(fam) == 2, log.kernels
            for p in range(batch):  # back through the single-modulus inverse of each polynomial
                sl = slice(p * n, (p + 1) * n)
                assert np.array_equal(cases[p % mc].gpu_inverse(np.array(got[sl])), x[sl])
