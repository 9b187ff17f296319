"""-m gpu: the four-polynomial tile of the forward 64-bit contiguous pass (ring 2^16, 10-stage last pass; csrc/
contig_p4_map.hpp, kern::merge_pass_lazy<..., P4>) against the CPU oracle, bit for bit, the way tests/test_gpu_merge.py
compares.  Every case runs with the test hook contig_p4 at 1 (four polynomials x one segment per tile) and at 0 (the
one-polynomial tile); both must give the oracle's words and enqueue kernels of the same names.  Batches that are no
multiple of 4 * mod_count take the one-polynomial tile whatever the hook says -- same words again."""
import os

import numpy as np
import pytest

from gpu_utils import MergeCase, find_ntt_factors, oracle_batch, rns_stack
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LOGN = 16
N = 1 << LOGN
MAX_BATCH = 12
# modulus -> lazy family of its kernels (the range behind the colon of the launch log)
FAMILIES = {"pool": 31, "b60": 0, "b61": 8, "b62": 4}


@pytest.fixture(scope="module")
def g(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    yield pkg
    pkg.set_test_hook("contig_p4", "1")


_cases = {}


def single_case(g, modulus, poly):
    """MergeCase + 12 distinct random polynomials + their oracle transforms, computed once per (modulus, polynomial)"""
    key = (modulus, poly)
    if key not in _cases:
        factors = None if modulus == "pool" else find_ntt_factors(int(modulus[1:]), LOGN, clear_of_top=True)
        c = MergeCase(g, 64, LOGN, poly, factors)
        x = c.random(MAX_BATCH, 0xC0F4 + len(_cases))
        want = oracle_batch([c], x)
        x.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (c, x, want)
    return _cases[key]


def check_per_polynomial(got, want, what):
    assert got.shape == want.shape
    for p in range(want.size // N):
        sl = slice(p * N, (p + 1) * N)
        if not np.array_equal(got[sl], want[sl]):
            # a polynomial that landed in another one's slot says so
            where = [r for r in range(want.size // N) if np.array_equal(got[sl], want[r * N:(r + 1) * N])]
            raise AssertionError("%s: output polynomial %d differs from the oracle (equals the oracle's polynomial %s)"
                                 % (what, p, where or "none"))


def both_tiles(g, run, want, what, launches, eligible=True):
    """run() with the hook at 1 and at 0: the oracle's words and the same kernel names both times.  The names cannot
    tell the tiles apart, the library's launch counter of the four-polynomial tile can: one launch per call with the
    hook at 1 when the batch is eligible, none otherwise"""
    logs = []
    try:
        for hook in ("1", "0"):
            g.set_test_hook("contig_p4", hook)
            before = g.contig_p4_launches()
            with g.launch_log() as log:
                got = run()
            took = g.contig_p4_launches() - before
            assert took == (1 if (hook == "1" and eligible) else 0), (what, hook, took)
            check_per_polynomial(got, want, "%s, contig_p4=%s" % (what, hook))
            logs.append(log.kernels)
    finally:
        g.set_test_hook("contig_p4", "1")
    assert logs[0] == logs[1] == launches, (what, logs)


@pytest.mark.parametrize("poly", [O.X_N_minus, O.X_N_plus])
@pytest.mark.parametrize("modulus", sorted(FAMILIES))
def test_forward_2_16_every_family_eligible_and_ineligible_batches(g, modulus, poly):
    """batches 4, 8, 12 (whole groups of four) and 5, 6 (the one-polynomial tile), in place and out of place, one
    modulus per lazy family, both reduction polynomials"""
    c, x, want = single_case(g, modulus, poly)
    k = "merge_pass_lazy:%d" % FAMILIES[modulus]
    for batch in (4, 8, 12, 5, 6):
        for inplace in (True, False):
            both_tiles(g, lambda: c.gpu_forward(np.array(x[:batch * N]), inplace=inplace), want[:batch * N],
                       (modulus, poly, batch, inplace), ["prep_twiddles", k, k], eligible=batch % 4 == 0)


def test_four_distinct_polynomials_each_checked_on_its_own(g):
    """a delta, a constant, q - 1 everywhere and random words: the four polynomials of ONE tile group are as different as
    polynomials get, so a lane map that permutes polynomials (or segments between them) cannot pass"""
    c, _, _ = single_case(g, "pool", O.X_N_plus)
    rows = [np.eye(1, N, 1)[0], np.ones(N), np.full(N, c.q - 1)]
    x = np.concatenate([np.asarray(r, dtype=object).astype(c.P.T) for r in rows] + [c.random(1, 77)])
    want = oracle_batch([c], x)
    assert len({want[p * N:(p + 1) * N].tobytes() for p in range(4)}) == 4
    for inplace in (True, False):
        both_tiles(g, lambda: c.gpu_forward(np.array(x), inplace=inplace), want, ("distinct", inplace),
                   ["prep_twiddles", "merge_pass_lazy:31", "merge_pass_lazy:31"])


def _rns_forward(g, cases, fwd, mods, x, batch, poly, inplace):
    import torch
    cfg = g.ntt_rns_configuration(n_power=LOGN, reduction_poly=poly)
    d = g.to_device(x)
    if inplace:
        g.GPU_NTT_Inplace(d, fwd, mods, cfg, batch, len(cases))
        out = d
    else:
        out = torch.zeros_like(d)
        g.GPU_NTT(d, out, fwd, mods, cfg, batch, len(cases))
    torch.cuda.synchronize()
    return g.to_host(out)


@pytest.mark.parametrize("widths,batch", [((60, 60), 8), ((60, 59, 58), 12), ((60, 59, 58), 8)])
def test_rns_stacks_share_a_modulus_inside_a_tile(g, widths, batch):
    """mod_count 2 with batch 8, mod_count 3 with batch 12 (the four polynomials of a tile lie 3 apart) and mod_count 3
    with batch 8 (no multiple of 12: the one-polynomial tile); drop-in call, moduli on the device"""
    poly = O.X_N_plus
    cases, fwd, _ = rns_stack(g, 64, LOGN, list(widths), poly)
    mc = len(cases)
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], 64)
    x = np.concatenate([cases[p % mc].P.splitmix(900 + p, 0, N, cases[p % mc].q) for p in range(batch)])
    want = oracle_batch(cases, x)
    g.set_test_hook("reset_predictions", "1")  # whatever stack lived at this address before
    _rns_forward(g, cases, fwd, mods, x, batch, poly, False)  # the family prediction of this stack settles here
    for inplace in (True, False):
        both_tiles(g, lambda: _rns_forward(g, cases, fwd, mods, x, batch, poly, inplace), want, (widths, batch, inplace),
                   ["prep_twiddles", "merge_pass_lazy:0", "merge_pass_lazy:0"], eligible=batch % (4 * mc) == 0)


@pytest.mark.parametrize("widths,family", [((60,), 0), ((62, 61), 4)])
def test_plan_execute_batch_8(g, widths, family):
    """NTTPlan.execute, batch 8: one modulus, and a stack of a 62- and a 61-bit prime (the 4 q kernels, moduli and
    normalisation constants per block from the plan's device arrays)"""
    import torch
    poly = O.X_N_minus
    cases, fwd, _ = rns_stack(g, 64, LOGN, list(widths), poly)
    mc, batch = len(cases), 8
    x = np.concatenate([cases[p % mc].P.splitmix(1700 + p, 0, N, cases[p % mc].q) for p in range(batch)])
    want = oracle_batch(cases, x)
    plan = g.NTTPlan(fwd, [c.prm.modulus for c in cases], LOGN, poly, g.FORWARD, batch_hint=batch)

    def run():
        d = g.to_device(x)
        out = torch.zeros_like(d)
        plan.execute(d, out, batch)
        torch.cuda.synchronize()
        return g.to_host(out)

    k = "merge_pass_lazy:%d" % family
    try:
        both_tiles(g, run, want, ("plan", widths), [k, k])
    finally:
        plan.close()
