"""KeySwitchPlan.rotate_hoisted_sum on the MI355X (include/gpuntt/rns/key_switch.cuh): the weighted sum of G rotations of
one decomposition, taken in the extended base before ONE ModDown.  Every comparison is torch.equal against the
definition -- hoisted_sum_utils.composition_sum, built from the calls that existed before -- on the same device data."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hoisted_sum_utils import composition_sum, make_weights, sum_scratch, with_nones
from hoisted_utils import any_words, canonical_key, device_words, elements_for, filled, make_plan, ring
from innerprod_utils import from_words, words
from keyswitch_utils import centre, crt, negacyclic, partition

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


@pytest.fixture
def chunk6(g):
    g.set_test_hook("keyswitch_hoist_chunk", 6)
    yield
    g.set_test_hook("keyswitch_hoist_chunk", 0)


def operands(g, plan, st, rng, count, G, km_moduli=None, offset=0):
    """a, c0 and G weights of arbitrary words, G canonical keys"""
    bits, n = plan.bits, 1 << plan.n_power
    L, M, D = plan.q_count, plan.mod_count, plan.digits
    a = device_words(g, any_words(g, rng, bits, D * count * M * n, st["moduli"]), offset)
    c0 = device_words(g, any_words(g, rng, bits, count * L * n, st["moduli"][:L]), offset)
    km = st["moduli"] if km_moduli is None else km_moduli
    keys = [device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset) for _ in range(G)]
    return a, c0, keys, make_weights(g, plan, st, rng, G, offset)


def weight_lists(weights):
    """per (with_c0, output_ntt) combination: the whole list None once, otherwise a list with at least one None entry
    at a position that moves -- except that with G = 1 the lone weight has to be present somewhere: there the list is
    [None] once and [w] twice"""
    G = len(weights)
    return {(False, False): None, (False, True): with_nones(weights, 0),
            (True, False): with_nones(weights, 1), (True, True): with_nones(weights, 2 if G > 2 else 1)}


def check_against_the_composition(g, plan, st, rng, combos, km_moduli=None, key_limbs=None, offset=0):
    import torch
    bits, n = plan.bits, 1 << plan.n_power
    L = plan.q_count
    for G, count in combos:
        elts = elements_for(g, plan.n_power, G)
        a, c0, keys, weights = operands(g, plan, st, rng, count, G, km_moduli, offset)
        keep = [t.clone() for t in (a, c0, *keys, *weights)]
        scratch = sum_scratch(plan, count)
        lists = weight_lists(weights)
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            w = lists[(with_c0, output_ntt)]
            want = composition_sum(g, plan, st, a, c0 if with_c0 else None, keys, elts, w, count, output_ntt, key_limbs)
            out = filled(bits, 2 * count * L * n, offset)
            plan.rotate_hoisted_sum(a, c0 if with_c0 else None, keys, elts, w, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (G, count, with_c0, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((a, c0, *keys, *weights), keep)), "an input was modified"


COMBOS = [(1, 1), (5, 3), (1, 3), (5, 1)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 6, 7, 9])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_with_chunks_of_64_slots(g, chunk6, bits, n_power, L, K, alpha, widths=None):
    """sub-chunk rings (one polynomial per workgroup, lanes without a slot), one chunk exactly, then 2 and 8 chunks: the
    source chunk differs per element, which is where a stale LDS tile or a missing barrier shows"""
    M = L + K
    st = ring(g, bits, n_power, widths=widths).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert g.keyswitch_hoist_sum_chunk(bits, plan.digits, n_power) == min(6, n_power)
    check_against_the_composition(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COMBOS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [6, 7])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_chunks_of_64_slots_on_the_widest_primes(g, chunk6, bits, n_power, L, K, alpha):
    """primes of 62/61 and 30/29 bits (hoisted_utils.WIDE_WIDTHS), one chunk exactly and two chunks: 2 q passes
    2^(W-1), where a signed comparison or a carry lost from the top bit shows"""
    test_every_output_word_with_chunks_of_64_slots(g, chunk6, bits, n_power, L, K, alpha, "wide")


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_with_the_automatic_chunk(g, bits, L, K, alpha, widths=None):
    n_power, M = 12, L + K
    st = ring(g, bits, n_power, widths=widths).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert n_power - g.keyswitch_hoist_sum_chunk(bits, plan.digits, n_power) >= 1  # at least 2 chunks per polynomial
    check_against_the_composition(g, plan, st, np.random.default_rng(L + bits), COMBOS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_the_automatic_chunk_on_the_widest_primes(g, bits, L, K, alpha):
    test_every_output_word_with_the_automatic_chunk(g, bits, L, K, alpha, "wide")


@pytest.mark.parametrize("bits", [64, 32])
def test_sixty_four_elements(g, chunk6, bits):
    n_power, L, K, alpha = 5, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(64 + bits), [(64, 1)])
    with pytest.raises(ValueError):
        a, c0, keys, weights = operands(g, plan, st, np.random.default_rng(1), 1, 1)
        plan.rotate_hoisted_sum(a, c0, keys * 65, [1] * 65, weights * 65, filled(bits, 2 * L << n_power), 1, False,
                                sum_scratch(plan, 1))


@pytest.mark.parametrize("bits", [64, 32])
def test_many_digits_force_a_small_chunk(g, bits, widths=None):
    """(L, K, alpha) = (20, 2, 1): D = 20, 21 rows of LDS per chunk slot"""
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K, widths=widths).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    # 21 rows x 256 slots x 8 bytes = 42 KiB is over the 32 KiB budget: 128 slots; 32-bit words fit 256
    assert plan.digits == 20 and g.keyswitch_hoist_sum_chunk(bits, 20, n_power) == (7 if bits == 64 else 8)
    check_against_the_composition(g, plan, st, np.random.default_rng(20 + bits), [(5, 3)])


@pytest.mark.parametrize("bits", [64, 32])
def test_many_digits_on_the_widest_primes(g, bits):
    test_many_digits_force_a_small_chunk(g, bits, "wide")


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, chunk6, bits):
    """a plan built with X_N_minus: elements reduced mod N, the cyclic slot order"""
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, poly=g.X_N_minus).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(6 + bits), [(5, 3)])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_keys_in_place(g, bits):
    """L = 4 of keys built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]; the weights have the
    plan's own M = 6 limbs in its own full-base order"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_against_the_composition(g, plan, st, np.random.default_rng(bits), [(5, 3)], km_moduli=full.moduli,
                                  key_limbs=limbs)


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """a, c0, the keys, the weights and out one word off 16-byte alignment (the scratch has to be 256-byte aligned)"""
    n_power, L, K, alpha = 7, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, _, _, weights = operands(g, plan, st, np.random.default_rng(1), 1, 1, offset=1)
    assert a.data_ptr() % 16 and weights[0].data_ptr() % 16
    check_against_the_composition(g, plan, st, np.random.default_rng(9 + bits), [(5, 3)], offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and the scratch inside larger sentinel-filled buffers; the inputs unmodified"""
    import torch
    n_power, L, K, alpha, G, count = 7, 3, 2, 2, 5, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, keys, weights = operands(g, plan, st, np.random.default_rng(bits), count, G)
    w = with_nones(weights, 3)
    keep = [t.clone() for t in (a, c0, *keys, *weights)]
    elts = elements_for(g, n_power, G)
    want = composition_sum(g, plan, st, a, c0, keys, elts, w, count, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = plan.hoisted_sum_scratch_bytes(count)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    plan.rotate_hoisted_sum(a, c0, keys, elts, w, big_out[pad:pad + words_out], count, True,
                            big_scratch[256:256 + sbytes])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())
    assert all(torch.equal(t, k) for t, k in zip((a, c0, *keys, *weights), keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_computes_a_linear_transform(g, bits):
    """The noiseless instance of test_gpu_hoisted_rotation.test_it_really_rotates: c0 + c1 s = msg (mod Q), and for k =
    rotation by 1 and conjugation a key that switches sigma_k(s) -> s, key_k[d] = (-a_d s + P g_d sigma_k(s), a_d),
    g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d].  The weights pt_g are small signed integer polynomials, reduced modulo all
    M moduli and transformed.  One decompose(c1), one rotate_hoisted_sum with both keys and both weights.

    Derivation of the bound.  As that test derives, the digits permuted by sigma_k are digits of sigma_k(c1) (the g_d
    sum absorbs whatever multiple of Q_d the ModUp added), so in the combination X_{g,0} + X_{g,1} s the accumulator of
    element g is P (sigma_k(c1) sigma_k(s) mod Q) + P sigma_k(c0) = P sigma_k(msg) (mod P Q), exactly: the key is
    noiseless and the c0 term is exact.  Multiplying by pt_g and summing over g happens in the ring mod P Q, word for
    word exact (canonical residues of exact sums), so the stack that reaches mod_down holds S_0, S_1 with
    S_0 + S_1 s = P sum_g pt_g sigma_k(msg) (mod P Q), whatever G and the pt_g are.  mod_down returns
    (S_c - [S_c]_P) / P per component, [.]_P the centred residue up to the rounding band: each of the TWO ModDowns is
    off from S_c / P by at most 1/2 + 3 K / 2^W per coefficient, and the combination (1, s) weighs them by
    |(1, s)|_1 = 1 + h, h = |s|_1.  The integer error of out_0 + out_1 s - sum_g pt_g sigma_k(msg), centred mod Q, is
    therefore at most (1 + h) / 2 + 1 -- the bound test_it_really_rotates has for ONE rotation.  It does not grow with
    G or with the weights because only one ModDown per component happens and the value before it is exact; the
    G-fold expression sum_g pt_g rotate_hoisted[g] would carry sum_g |pt_g|_1 times that."""
    import torch
    n_power, L, K, alpha = 5, 3, 2, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    full, qs, ps = st["moduli"], st["moduli"][:L], st["moduli"][L:]
    Q, P = math.prod(qs), math.prod(ps)
    plan = make_plan(g, st, L, alpha, n_power, bits)
    rng = np.random.default_rng(23 + bits)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    h = int(sum(abs(v) for v in s))
    elts = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_conjugation(n_power)]

    def sigma(x, k):  # a(X) -> a(X^k) in Z[X] / (X^N + 1)
        out = np.zeros(n, dtype=object)
        for i in range(n):
            e = (i * k) % (2 * n)
            out[e % n] += x[i] if e < n else -x[i]
        return out

    parts = partition(L, alpha)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)
    keys, weights, pts = [], [], []
    for k in elts:
        key = np.zeros((len(parts), 2, M, n), dtype=object)
        for d, S in enumerate(parts):
            Qd = math.prod(qs[i] for i in S)
            gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
            a_d = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(n)], dtype=object)
            b_d = -negacyclic(a_d, s) + P * gd * sigma(s, k)
            for m, q in enumerate(full):
                key[d, 0, m], key[d, 1, m] = b_d % q, a_d % q
        d_key = device_words(g, words(g, key, bits))
        g.GPU_NTT_Inplace(d_key, st["fwd"], st["mods"], cfg_f, len(parts) * 2 * M, M)
        keys.append(d_key)
        pt = np.array([int(v) for v in rng.integers(-50, 51, size=n)], dtype=object)
        d_pt = device_words(g, words(g, np.array([pt % q for q in full], dtype=object), bits))
        g.GPU_NTT_Inplace(d_pt, st["fwd"], st["mods"], cfg_f, M, M)
        weights.append(d_pt), pts.append(pt)
    c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
    msg = np.array([int(v) for v in rng.integers(-1000, 1000, size=n)], dtype=object)
    c0 = (msg - negacyclic(c1, s)) % Q
    d_c1 = device_words(g, words(g, np.array([c1 % q for q in qs], dtype=object), bits))
    d_c0 = device_words(g, words(g, np.array([c0 % q for q in qs], dtype=object), bits))
    g.GPU_NTT_Inplace(d_c0, st["fwd"], st["mods"], cfg_f, L, L)
    a = filled(bits, plan.digits * M * n)
    plan.decompose(d_c1, a, 1, False, None)
    out = filled(bits, 2 * L * n)
    plan.rotate_hoisted_sum(a, d_c0, keys, elts, weights, out, 1, False, sum_scratch(plan, 1))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    bound = (1 + h) / 2 + 1
    want = sum(negacyclic(pt, sigma(msg, k)) for pt, k in zip(pts, elts))
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    err = [abs(int(v)) for v in centre((value - want) % Q, Q)]
    print("largest error %d, bound %.1f" % (max(err), bound))
    assert max(err) <= bound, (max(err), bound)


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha, count = 64, 9, 6, 2, 2, 3
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, keys, weights = operands(g, plan, st, np.random.default_rng(5), count, 5)
    mods = [c.prm.modulus for c in full.cases[:M]]
    out = filled(bits, 2 * count * L * n)
    # the scratch does not grow with G and is smaller than a: it is the head of a buffer long enough to pose as a
    sbytes = plan.hoisted_sum_scratch_bytes(count)
    big = torch.zeros(max(sbytes, a.numel() * 8), dtype=torch.uint8, device="cuda:0")
    scratch = big[:sbytes]
    assert scratch.data_ptr() % 256 == 0
    stages = {}
    for name, table, kind, mc, buf in (("inv_full", st["inv"], g.INVERSE, M, scratch.view(torch.int64)),
                                       ("fwd_q", st["fwd"], g.FORWARD, L, out)):
        alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
        with g.launch_log() as log:
            alone.execute(buf, buf, 2 * count * mc)
        stages[name] = log.kernels
        assert log.kernels
    torch.cuda.synchronize()
    for G in (1, 5):
        elts = elements_for(g, n_power, G)
        w = with_nones(weights[:G], 1)
        before = torch.cuda.memory_allocated()
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            with g.launch_log() as log:
                plan.rotate_hoisted_sum(a, c0 if with_c0 else None, keys[:G], elts, w, out, count, output_ntt, scratch)
            want = ["inner_product_galois_sum"] + stages["inv_full"] + ["base_convert"] + \
                (stages["fwd_q"] if output_ntt else [])
            assert log.kernels == want, (log.kernels, want)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    G = 5
    with g.launch_log() as log:
        plan.rotate_hoisted_sum(a, c0, keys, elts, weights, out, 0, True, scratch)
    assert log.kernels == []
    tail = scratch.view(torch.int64)
    off = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    call, ws = plan.rotate_hoisted_sum, weights
    refused = [lambda: call(a, c0, [], [], [], out, count, False, scratch),                        # G = 0
               lambda: call(a, c0, keys * 13, elts * 13, ws * 13, out, count, False, scratch),     # G = 65
               lambda: call(a, c0, keys * 13, elts * 13, None, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, ws, out, -1, False, scratch),
               lambda: call(a, c0, keys, elts[:4] + [2], ws, out, count, False, scratch),          # an even element
               lambda: call(a, c0, keys, elts[:4] + [2 << n_power], ws, out, count, False, scratch),  # even once reduced
               lambda: call(None, c0, keys, elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, ws, None, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [None], elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, ws, out, count, False, None),
               lambda: call(a, c0, keys[:4], elts, ws, out, count, False, scratch),                # one key per element
               lambda: call(a, c0, keys, elts, ws[:4], out, count, False, scratch),                # one weight per element
               lambda: call(a, c0, keys, elts, ws, out, count, False, sum_scratch(plan, count, short=1)),
               lambda: call(a, c0, keys, elts, ws, out, count, False, off[8:]),                    # not 256-byte aligned
               lambda: call(a[1:], c0, keys, elts, ws, out, count, False, scratch),                # too small
               lambda: call(a, c0[1:], keys, elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [keys[4][1:]], elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, ws[:4] + [ws[4][1:]], out, count, False, scratch),  # a weight too small
               lambda: call(a, c0, keys, elts, ws, out[1:], count, False, scratch),
               lambda: call(a.to(torch.int32), c0, keys, elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, [None] * 4 + [ws[4].to(torch.int32)], out, count, False, scratch),
               # out or the scratch over a, c0, a key, a weight or each other
               lambda: call(big.view(torch.int64)[:a.numel()], c0, keys, elts, ws, out, count, False, scratch),
               lambda: call(a, tail[-c0.numel():], keys, elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [tail[:keys[0].numel()]], elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, [None] * 4 + [tail[-ws[0].numel():]], out, count, False, scratch),
               lambda: call(a, c0, keys, elts, ws, tail[-out.numel():], count, False, scratch),
               lambda: call(out[:a.numel()], c0, keys, elts, ws, out, count, False, scratch),
               lambda: call(a, out[-c0.numel():], keys, elts, ws, out, count, False, scratch),
               lambda: call(a, c0, [out[:keys[0].numel()]] + keys[1:], elts, ws, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, [out[:ws[0].numel()]] + ws[1:], out, count, False, scratch),
               lambda: bare.rotate_hoisted_sum(a, c0, keys, elts, ws, out, count, False, scratch)]  # no transforms
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """one stream, a linear capture (no parallel branches), replayed twice with new data"""
    import torch
    n_power, L, K, alpha, G, count = 9, 3, 2, 2, 3, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    elts = elements_for(g, n_power, G)
    a, c0, keys, weights = operands(g, plan, st, np.random.default_rng(0), count, G)
    w = with_nones(weights, 1)
    out = filled(bits, 2 * count * L * n)
    scratch, scratch2 = sum_scratch(plan, count), sum_scratch(plan, count)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.rotate_hoisted_sum(a, c0, keys, elts, w, out, count, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.rotate_hoisted_sum(a, c0, keys, elts, w, out, count, True, scratch, stream=s)
    for seed in (1, 2):
        na, nc0, nkeys, nweights = operands(g, plan, st, np.random.default_rng(seed), count, G)
        a.copy_(na), c0.copy_(nc0)
        for k, nk in zip(keys + weights, nkeys + nweights):
            k.copy_(nk)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = filled(bits, 2 * count * L * n)
        plan.rotate_hoisted_sum(a, c0, keys, elts, w, eager, count, True, scratch2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed
        assert torch.equal(eager, composition_sum(g, plan, st, a, c0, keys, elts, w, count, True)), seed


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_hoisted_sum.cpp, compiled here against include/ and libgpuntt.so: the weighted sum of three
    rotations of one ciphertext from one decompose, compared with the composition"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_hoisted_sum")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_hoisted_sum.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
