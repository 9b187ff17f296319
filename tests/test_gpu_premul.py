"""-m gpu: the hoisted first twiddle product of the forward 64-bit ring 2^16 (csrc/contig_p4_map.hpp: premul; kern::
pass_body<..., PRE>) against the CPU oracle, bit for bit, the way tests/test_gpu_contig_p4.py compares.  With the test
hook premul at 1 the strided pass multiplies the bit-9 half of the ring by the last pass's first-stage twiddles and the
four-polynomial last pass starts from the products; at 0 both passes run as before.  Both must give the oracle's words
under the same kernel names, and the library's counter must move exactly when the call is eligible (a plain forward
call or plan whose last pass takes the four-polynomial tile, 31 q / 16 q families) and the hook is 1.  Calls that run the
one-polynomial tile (batch 5, *_Poly_Ordered, the fused product of GPU_PolyMul) have no such variant: same words, and
the counter stays."""
import os

import numpy as np
import pytest

from gpu_utils import MergeCase, _is_probable_prime, find_ntt_factors, oracle_batch, rns_stack
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LOGN = 16
N = 1 << LOGN
MAX_BATCH = 8
DEFAULT_HOOK = "1"
# modulus -> lazy family of its kernels (the range behind the colon of the launch log)
FAMILIES = {"pool": 31, "w31": 31, "b60": 0}


def widest_31q_factors(logn):
    """(q, omega, psi) of the largest NTT prime with 31 q < 2^64: the top of the 31 q family's range"""
    step = 1 << (logn + 1)
    q = ((1 << 64) - 1) // 31 // step * step + 1
    while q > ((1 << 64) - 1) // 31 or not _is_probable_prime(q):
        q -= step
    assert 31 * q < 1 << 64 and 32 * q > 1 << 64
    gen = 2
    while True:
        psi = pow(gen, (q - 1) >> (logn + 1), q)
        if pow(psi, 1 << logn, q) == q - 1:
            return q, psi * psi % q, psi
        gen += 1


@pytest.fixture(scope="module")
def g(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    yield pkg
    pkg.set_test_hook("premul", DEFAULT_HOOK)


_cases = {}


def patterns(c, seed):
    """eight polynomials; the first four (one tile group) are random residues, all zero, all q - 1, and q - 1 on the
    bit-9 half of the ring only (the positions the strided pass multiplies)"""
    x = np.array(c.random(MAX_BATCH, seed))
    x[N:2 * N] = 0
    x[2 * N:3 * N] = c.q - 1
    half = ((np.arange(N) >> 9) & 1).astype(bool)
    x[3 * N:4 * N] = np.where(half, np.array(c.q - 1, dtype=x.dtype), np.array(0, dtype=x.dtype))
    return x


def single_case(g, modulus, poly):
    key = (modulus, poly)
    if key not in _cases:
        factors = {"pool": None, "w31": widest_31q_factors(LOGN),
                   "b60": find_ntt_factors(60, LOGN, clear_of_top=True)}[modulus]
        if modulus == "b60":
            assert 31 * factors[0] >= 1 << 64  # outside the 31 q family
        c = MergeCase(g, 64, LOGN, poly, factors)
        x = patterns(c, 0x9E61 + len(_cases))
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
            bad = np.flatnonzero(got[sl] != want[sl])
            raise AssertionError("%s: output polynomial %d differs from the oracle at %d positions, first %d"
                                 % (what, p, bad.size, bad[0]))


def both_hooks(g, run, want, what, eligible, launches=None, counted=True):
    """run() with the hook at 1 and at 0: the oracle's words (want) both times and, where asked, the same kernel names;
    the counter moves exactly when the call is eligible and the hook is 1"""
    outs, logs = [], []
    try:
        for hook in ("1", "0"):
            g.set_test_hook("premul", hook)
            before = g.premul_launches()
            with g.launch_log() as log:
                got = run()
            moved = g.premul_launches() - before
            if counted:
                assert (moved > 0) == (eligible and hook == "1"), (what, "premul=" + hook, moved)
            if want is not None:
                check_per_polynomial(got, want, "%s, premul=%s" % (what, hook))
            outs.append(got)
            logs.append(log.kernels)
    finally:
        g.set_test_hook("premul", DEFAULT_HOOK)
    assert np.array_equal(outs[0], outs[1]), (what, "the hook changes the words")
    assert logs[0] == logs[1], (what, logs)
    if launches is not None:
        assert logs[0] == launches, (what, logs)


@pytest.mark.parametrize("poly", [O.X_N_minus, O.X_N_plus])
@pytest.mark.parametrize("modulus", sorted(FAMILIES))
def test_forward_2_16_dropin(g, modulus, poly):
    """batches 4 and 8, in place and out of place, the pool prime, the widest 31 q prime and a 60-bit prime; batch 5
    (the one-polynomial tile) keeps the plain strided kernel"""
    c, x, want = single_case(g, modulus, poly)
    k = "merge_pass_lazy:%d" % FAMILIES[modulus]
    for batch in (4, 8, 5):
        for inplace in (True, False):
            both_hooks(g, lambda: c.gpu_forward(np.array(x[:batch * N]), inplace=inplace), want[:batch * N],
                       (modulus, poly, batch, inplace), eligible=batch % 4 == 0, launches=["prep_twiddles", k, k])


@pytest.mark.parametrize("modulus", sorted(FAMILIES))
def test_forward_2_16_plan(g, modulus):
    """NTTPlan.execute, batches 4 and 8, out of place and in place, both reduction polynomials"""
    import torch
    k = "merge_pass_lazy:%d" % FAMILIES[modulus]
    for poly in (O.X_N_minus, O.X_N_plus):
        c, x, want = single_case(g, modulus, poly)
        plan = g.NTTPlan(c.fwd_dev, c.prm.modulus, LOGN, poly, g.FORWARD, batch_hint=MAX_BATCH)
        try:
            for batch in (4, 8):
                for inplace in (True, False):
                    def run():
                        d = g.to_device(np.array(x[:batch * N]))
                        out = d if inplace else torch.zeros_like(d)
                        plan.execute(d, out, batch)
                        torch.cuda.synchronize()
                        return g.to_host(out)
                    both_hooks(g, run, want[:batch * N], ("plan", modulus, poly, batch, inplace), eligible=True,
                               launches=[k, k])
        finally:
            plan.close()


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


@pytest.mark.parametrize("widths,family", [((60, 60), 0), ((59, 58), None)])
def test_rns_stack_of_two_primes_batch_8(g, widths, family):
    """drop-in call, moduli on the device: polynomial p uses prime p % 2 and that prime's slot of the twiddle table"""
    poly = O.X_N_plus
    cases, fwd, _ = rns_stack(g, 64, LOGN, list(widths), poly)
    mc, batch = len(cases), 8
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], 64)
    x = np.concatenate([cases[p % mc].P.splitmix(4100 + p, 0, N, cases[p % mc].q) for p in range(batch)])
    for p in (2, 3):  # q - 1 everywhere, one polynomial per prime
        x[p * N:(p + 1) * N] = cases[p % mc].q - 1
    want = oracle_batch(cases, x)
    g.set_test_hook("reset_predictions", "1")  # whatever stack lived at this address before
    for _ in range(2):
        _rns_forward(g, cases, fwd, mods, x, batch, poly, False)  # the family prediction of this stack settles here
    # (60, 60): the 16 q family, pinned by name; (59, 58): whichever of the two families the prediction settled on
    k = "merge_pass_lazy:%d" % family if family is not None else None
    for inplace in (True, False):
        both_hooks(g, lambda: _rns_forward(g, cases, fwd, mods, x, batch, poly, inplace), want, (widths, inplace),
                   eligible=True, launches=["prep_twiddles", k, k] if k else None)


def test_poly_ordered_and_polymul_keep_their_words(g):
    """a *_Poly_Ordered call and GPU_PolyMul run the one-polynomial tile: the hook changes no word.  The ordered call
    never counts; GPU_PolyMul is compared word for word only (its unfused forward transform is a plain call)"""
    import torch
    poly = O.X_N_plus
    cases, fwd, _ = rns_stack(g, 64, LOGN, [60, 60], poly)
    mc, batch, stored = 2, 8, 9
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], 64)
    slots = [8, 4, 7, 3, 0, 6, 1, 2]
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
    buf = np.zeros(stored * N, dtype=cases[0].P.T)
    for p, sl in enumerate(slots):
        buf[sl * N:(sl + 1) * N] = cases[p % mc].P.splitmix(5200 + p, 0, N, cases[p % mc].q)
    buf[5 * N:6 * N] = 12345
    want = buf.copy()
    for p, sl in enumerate(slots):
        want[sl * N:(sl + 1) * N] = cases[p % mc].P.merge_ntt(buf[sl * N:(sl + 1) * N], cases[p % mc].oprm)
    cfg = g.ntt_rns_configuration(n_power=LOGN, ntt_type=g.FORWARD, reduction_poly=poly)

    def ordered():
        d = g.to_device(buf)
        g.GPU_NTT_Poly_Ordered(d, d, fwd, mods, cfg, batch, mc, d_slots)
        torch.cuda.synchronize()
        return g.to_host(d)

    ordered()  # the family prediction settles
    both_hooks(g, ordered, want, "poly-ordered", eligible=False)

    c, x, _ = single_case(g, "pool", O.X_N_plus)

    def polymul():
        da, db = g.to_device(np.array(x[:4 * N])), g.to_device(np.array(x[4 * N:8 * N]))
        out = torch.zeros_like(da)
        g.GPU_PolyMul(da, db, out, c.fwd_dev, c.inv_dev, c.prm.modulus, c.cfg(inverse=True), 4)
        torch.cuda.synchronize()
        return g.to_host(out)

    both_hooks(g, polymul, None, "polymul", eligible=False, counted=False)


@pytest.mark.parametrize("modulus", sorted(FAMILIES))
def test_forward_then_inverse_returns_the_input(g, modulus):
    c, x, want = single_case(g, modulus, O.X_N_plus)
    g.set_test_hook("premul", "1")
    try:
        before = g.premul_launches()
        y = c.gpu_forward(np.array(x[:4 * N]), inplace=True)
        assert g.premul_launches() - before == 1
        assert np.array_equal(c.gpu_inverse(y, inplace=True), x[:4 * N])
    finally:
        g.set_test_hook("premul", DEFAULT_HOOK)
