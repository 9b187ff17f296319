"""KeySwitchPlan.multiply_relinearize_sum on the MI355X (include/gpuntt/rns/key_switch.cuh): sum_t x_t y_t over T pairs of
ciphertexts with one key switch and one ModDown.  Every comparison is torch.equal against the definition --
relin_sum_utils.composition_relin_sum, built from the calls that existed before -- on the same device data, or
array_equal against relin_sum_exact's Python integers."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hoisted_exact import host_cases
from hoisted_utils import WIDE_WIDTHS, device_words, filled, make_plan, ring
from innerprod_utils import from_words, words
from keyswitch_utils import centre, crt, negacyclic, partition
from relin_sum_exact import exact_multiply_relinearize_sum
from relin_sum_utils import composition_relin_sum, relin_sum_operands
from relin_utils import relin_scratch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = (1, 3, 5)  # RB = 1; 2 with a ragged tail, in two and in three blocks
TERMS = (1, 2, 3)
SHAPES = [(3, 2, 2), (6, 2, 2)]


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def check_against_the_composition(g, plan, st, rng, counts, terms_of, km_moduli=None, offset=0):
    import torch
    bits, n, L = plan.bits, 1 << plan.n_power, plan.q_count
    for count in counts:
        scratch = relin_scratch(plan, count)
        for terms in terms_of:
            xs, ys, key = relin_sum_operands(g, plan, st, rng, count, terms, km_moduli, offset)
            keep = [t.clone() for t in xs + ys + [key]]
            for output_ntt in (False, True):
                want = composition_relin_sum(g, plan, st, xs, ys, key, count, output_ntt)
                out = filled(bits, 2 * count * L * n, offset)
                plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
                torch.cuda.synchronize()
                assert torch.equal(out, want), (count, terms, output_ntt)
            assert all(torch.equal(t, k) for t, k in zip(xs + ys + [key], keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9, 12])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_every_output_word(g, bits, n_power, L, K, alpha):
    """N = 2 at u32 is below a 16-byte group: the one-word loader; 2^12 has several column tiles per polynomial"""
    M = L + K
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COUNTS, TERMS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 12])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_one_term_equals_multiply_relinearize(g, bits, n_power, L, K, alpha):
    """terms = 1 is multiply_relinearize's definition: the same words from both calls on the same data"""
    import torch
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    rng = np.random.default_rng(n_power + L + bits)
    for count in COUNTS:
        xs, ys, key = relin_sum_operands(g, plan, st, rng, count, 1)
        scratch = relin_scratch(plan, count)
        for output_ntt in (False, True):
            one, out = filled(bits, 2 * count * L * n), filled(bits, 2 * count * L * n)
            plan.multiply_relinearize(xs[0], ys[0], key, one, count, output_ntt, scratch)
            plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, one), (count, output_ntt)


@pytest.mark.parametrize("bits", [64, 32])
def test_thirty_two_terms(g, bits):
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(32 + bits), [1, 5], [32])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [6, 12])
@pytest.mark.parametrize("widths", ["wide", "spread"])
def test_every_output_word_on_the_widest_primes(g, bits, n_power, widths):
    """primes of 62/61 and 30/29 bits, and primes spread over the eighth below 2^(W-2): there the fold sum reaches
    [2^(W-1), 3 q), where a signed comparison or a carry lost from the top bit shows"""
    L, K, alpha = 3, 2, 2
    st = ring(g, bits, n_power, widths=widths).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(n_power + L + bits), COUNTS, [3])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,count,terms,ones", [(5, 3, 3, False), (7, 3, 3, False), (5, 2, 32, True)])
def test_against_exact_integers_on_the_widest_primes(g, bits, n_power, count, terms, ones):
    """relin_sum_exact: no GPU call and none of the library's arithmetic.  ones: every operand word is 2^W - 1 at
    terms = 32, the largest carry count the accumulators can be given"""
    import torch
    L, K, alpha = 3, 2, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power, widths="wide").sub(list(range(M)))
    cases = host_cases(bits, n_power, WIDE_WIDTHS[bits], M)
    assert [c.q for c in cases] == st["moduli"]
    plan = make_plan(g, st, L, alpha, n_power, bits)
    xs, ys, key = relin_sum_operands(g, plan, st, np.random.default_rng(bits + n_power), count, terms)
    if ones:
        for t in xs + ys:
            t.fill_(-1)
    hx = [from_words(g.to_host(t), (2, count, L, n)) for t in xs]
    hy = [from_words(g.to_host(t), (2, count, L, n)) for t in ys]
    if ones:
        assert all(int(v) == (1 << bits) - 1 for h in hx + hy for v in h.reshape(-1)[:3])
    hkey = from_words(g.to_host(key), (plan.digits, 2, M, n))
    scratch = relin_scratch(plan, count)
    for output_ntt in (False, True):
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        want = exact_multiply_relinearize_sum(cases, L, alpha, bits, hx, hy, hkey, output_ntt)
        assert np.array_equal(from_words(g.to_host(out), want.shape), want), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
def test_twenty_digits(g, bits):
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert plan.digits == 20
    check_against_the_composition(g, plan, st, np.random.default_rng(20 + bits), [3], [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, bits):
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, poly=g.X_N_minus).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(6 + bits), [3], [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_key_in_place(g, bits):
    """L = 4 of a key built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_against_the_composition(g, plan, st, np.random.default_rng(bits), [3], [3], km_moduli=full.moduli)


@pytest.mark.parametrize("bits", [64, 32])
def test_squares_shared_tensors_and_out_over_an_operand(g, bits):
    """y[t] is x[t] for all t; one tensor in two terms; out given as x[0], then as y[T - 1] -- each compared with the
    result into a separate buffer"""
    import torch
    n_power, L, K, alpha, count, T = 9, 3, 2, 2, 3, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    xs, ys, key = relin_sum_operands(g, plan, st, np.random.default_rng(3 + bits), count, T)
    scratch = relin_scratch(plan, count)
    for output_ntt in (False, True):
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize_sum(xs, xs, key, out, count, output_ntt, scratch)  # squares
        torch.cuda.synchronize()
        assert torch.equal(out, composition_relin_sum(g, plan, st, xs, xs, key, count, output_ntt)), output_ntt
        shared_x, shared_y = [xs[0], xs[1], xs[0]], [ys[0], ys[1], xs[1]]  # xs[0] in two terms, xs[1] on both sides
        plan.multiply_relinearize_sum(shared_x, shared_y, key, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(out, composition_relin_sum(g, plan, st, shared_x, shared_y, key, count, output_ntt))
        plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
        x0, yl = xs[0].clone(), ys[T - 1].clone()
        plan.multiply_relinearize_sum([x0] + xs[1:], ys, key, x0, count, output_ntt, scratch)
        plan.multiply_relinearize_sum(xs, ys[:T - 1] + [yl], key, yl, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(x0, out) and torch.equal(yl, out), output_ntt
        sq = [t.clone() for t in xs]
        plan.multiply_relinearize_sum(sq, sq, key, sq[1], count, output_ntt, scratch)  # squares, in place over one
        torch.cuda.synchronize()
        assert torch.equal(sq[1], composition_relin_sum(g, plan, st, xs, xs, key, count, output_ntt)), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_of_one_term_one_word_off_alignment(g, bits):
    """x and y of the middle term one word off 16-byte alignment, everything else aligned (the whole launch takes the
    one-word loader); then every operand, the key and out off"""
    import torch
    n_power, L, K, alpha, T = 7, 3, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    rng = np.random.default_rng(9 + bits)
    for count in COUNTS:
        xs, ys, key = relin_sum_operands(g, plan, st, rng, count, T)
        off_x, off_y, _ = relin_sum_operands(g, plan, st, rng, count, 1, offset=1)
        xs[1], ys[1] = off_x[0], off_y[0]
        assert xs[1].data_ptr() % 16 and ys[1].data_ptr() % 16 and not xs[0].data_ptr() % 16 and not key.data_ptr() % 16
        scratch = relin_scratch(plan, count)
        for output_ntt in (False, True):
            out = filled(bits, 2 * count * L * n)
            plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, composition_relin_sum(g, plan, st, xs, ys, key, count, output_ntt)), (count, output_ntt)
    check_against_the_composition(g, plan, st, rng, [3], [2], offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and the scratch inside larger sentinel-filled buffers; the inputs unmodified"""
    import torch
    n_power, L, K, alpha, count, T = 7, 3, 2, 2, 3, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    xs, ys, key = relin_sum_operands(g, plan, st, np.random.default_rng(bits), count, T)
    keep = [t.clone() for t in xs + ys + [key]]
    want = composition_relin_sum(g, plan, st, xs, ys, key, count, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = plan.scratch_bytes(count, 2)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    plan.multiply_relinearize_sum(xs, ys, key, big_out[pad:pad + words_out], count, True, big_scratch[256:256 + sbytes])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())
    assert all(torch.equal(t, k) for t, k in zip(xs + ys + [key], keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_multiplies_and_sums(g, bits):
    """A noiseless instance, built as test_gpu_relin.test_it_really_multiplies builds it: ternary s with h = |s|_1, 2 T
    ciphertexts with c0 + c1 s = msg exactly (mod Q), |msg| < 1000, T = 3, and a key that switches s^2 -> s,
    key[d] = (-a_d s + P g_d s^2, a_d), g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d].

    Derivation of the bound: that of ONE product.  The digits of d2 = sum_t x1_t y1_t (mod Q) are digits of that
    polynomial (the g_d sum absorbs whatever multiple of Q_d the ModUp added), so the accumulators of the switch satisfy
    A_0 + A_1 s = P d2 s^2 (mod P Q) exactly: the key is noiseless.  The summed tensor terms join as P d0 and P d1, exact
    residues, so the stack that reaches mod_down holds S_0 + S_1 s = P (d0 + d1 s + d2 s^2) = P sum_t msg_x_t msg_y_t
    (mod P Q) -- the sum was taken BEFORE the rounding.  mod_down returns (S_c - [S_c]_P) / P per component: each of the
    TWO ModDowns is off from S_c / P by at most 1/2 + 3 K / 2^W per coefficient, and the combination (1, s) weighs them
    by 1 + h.  The centred error of out_0 + out_1 s - sum_t msg_x_t msg_y_t is therefore at most (1 + h) / 2 + 1, whatever
    T is; T calls of multiply_relinearize would carry T times that."""
    import torch
    n_power, L, K, alpha, T = 5, 3, 2, 2, 3
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    full, qs, ps = st["moduli"], st["moduli"][:L], st["moduli"][L:]
    Q, P = math.prod(qs), math.prod(ps)
    plan = make_plan(g, st, L, alpha, n_power, bits)
    rng = np.random.default_rng(31 + bits)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    h = int(sum(abs(v) for v in s))
    s2 = negacyclic(s, s)
    parts = partition(L, alpha)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)
    key = np.zeros((len(parts), 2, M, n), dtype=object)
    for d, S in enumerate(parts):
        Qd = math.prod(qs[i] for i in S)
        gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
        a_d = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(n)], dtype=object)
        b_d = -negacyclic(a_d, s) + P * gd * s2
        for m, q in enumerate(full):
            key[d, 0, m], key[d, 1, m] = b_d % q, a_d % q
    d_key = device_words(g, words(g, key, bits))
    g.GPU_NTT_Inplace(d_key, st["fwd"], st["mods"], cfg_f, len(parts) * 2 * M, M)
    cts, msgs = [], []
    for _ in range(2 * T):
        c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
        msg = np.array([int(v) for v in rng.integers(-999, 1000, size=n)], dtype=object)
        c0 = (msg - negacyclic(c1, s)) % Q
        ct = device_words(g, words(g, np.array([[c % q for q in qs] for c in (c0, c1)], dtype=object), bits))
        g.GPU_NTT_Inplace(ct, st["fwd"], st["mods"], cfg_f, 2 * L, L)
        cts.append(ct), msgs.append(msg)
    out = filled(bits, 2 * L * n)
    plan.multiply_relinearize_sum(cts[:T], cts[T:], d_key, out, 1, False, relin_scratch(plan, 1))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    bound = (1 + h) / 2 + 1
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    exact = sum(negacyclic(msgs[t], msgs[T + t]) for t in range(T))
    err = [abs(int(v)) for v in centre((value - exact) % Q, Q)]
    print("largest error %d, bound %.1f" % (max(err), bound))
    assert max(err) <= bound, (max(err), bound)


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha, count, T = 64, 9, 6, 2, 2, 3, 3
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    xs, ys, key = relin_sum_operands(g, plan, st, np.random.default_rng(5), count, T)
    mods = [c.prm.modulus for c in full.cases[:M]]
    out = filled(bits, 2 * count * L * n)
    sbytes = plan.scratch_bytes(count, 2)
    big = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    scratch = big[:sbytes]
    assert scratch.data_ptr() % 256 == 0
    words64 = scratch.view(torch.int64)
    stages = {}
    for name, table, kind, mc, batch in (("inv_q", st["inv"], g.INVERSE, L, count * L),
                                         ("fwd_full", st["fwd"], g.FORWARD, M, D * count * M),
                                         ("inv_full", st["inv"], g.INVERSE, M, 2 * count * M),
                                         ("fwd_q", st["fwd"], g.FORWARD, L, 2 * count * L)):
        alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
        buf = words64[:batch * n]
        with g.launch_log() as log:
            alone.execute(buf, buf, batch)
        stages[name] = log.kernels
        assert log.kernels
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for output_ntt in (False, True):
        with g.launch_log() as log:
            plan.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch)
        want = ["tensor_top_sum"] + stages["inv_q"] + ["ks_mod_up"] + stages["fwd_full"] + \
            ["inner_product_tensor_sum"] + stages["inv_full"] + ["base_convert"] + (stages["fwd_q"] if output_ntt else [])
        assert log.kernels == want, (log.kernels, want)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    with g.launch_log() as log:
        plan.multiply_relinearize_sum(xs, ys, key, out, 0, True, scratch)
    assert log.kernels == []
    off = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    ct = xs[0].numel()
    pair = filled(bits, ct + 8)  # two ciphertexts 8 words apart: an overlap that is not "exactly"
    call = plan.multiply_relinearize_sum
    refused = [lambda: call(None, ys, key, out, count, False, scratch),
               lambda: call(xs, None, key, out, count, False, scratch),
               lambda: call([], [], key, out, count, False, scratch),
               lambda: call(xs, ys[:2], key, out, count, False, scratch),
               lambda: call(xs * 11, ys * 11, key, out, count, False, scratch),           # terms = 33
               lambda: call([xs[0], None, xs[2]], ys, key, out, count, False, scratch),
               lambda: call(xs, [ys[0], ys[1], None], key, out, count, False, scratch),
               lambda: call(xs, ys, None, out, count, False, scratch),
               lambda: call(xs, ys, key, None, count, False, scratch),
               lambda: call(xs, ys, key, out, count, False, None),
               lambda: call(xs, ys, key, out, -1, False, scratch),
               lambda: call(xs, ys, key, out, 1 << 24, False, scratch),                 # beyond every buffer and limit
               lambda: call(xs, ys, key, out, count, False, relin_scratch(plan, count, short=1)),
               lambda: call(xs, ys, key, out, count, False, off[8:]),                   # not 256-byte aligned
               lambda: call([xs[0], xs[1][1:], xs[2]], ys, key, out, count, False, scratch),  # too small
               lambda: call(xs, [ys[0][1:], ys[1], ys[2]], key, out, count, False, scratch),
               lambda: call(xs, ys, key[1:], out, count, False, scratch),
               lambda: call(xs, ys, key, out[1:], count, False, scratch),
               lambda: call([xs[0], xs[1].to(torch.int32), xs[2]], ys, key, out, count, False, scratch),
               # out over one x[t] or y[t], but not exactly; out over the key; out or the scratch over an operand or each
               # other
               lambda: call([xs[0], pair[:ct], xs[2]], ys, key, pair[8:], count, False, scratch),
               lambda: call(xs, [ys[0], ys[1], pair[8:]], key, pair[:ct], count, False, scratch),
               lambda: call(xs, ys, key, key[:ct], count, False, scratch),
               lambda: call([xs[0], xs[1], words64[:ct]], ys, key, out, count, False, scratch),
               lambda: call(xs, [words64[-ct:], ys[1], ys[2]], key, out, count, False, scratch),
               lambda: call(xs, ys, words64[:key.numel()], out, count, False, scratch),
               lambda: call(xs, ys, key, words64[-ct:], count, False, scratch),
               lambda: bare.multiply_relinearize_sum(xs, ys, key, out, count, False, scratch)]  # no transforms
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    # the library's own refusals of what the wrapper stops first: terms outside [1, 32], a null array, a null entry
    fn = g.load_library().gpuntt_keyswitch_plan_multiply_relinearize_sum_u64

    def ptrs(ts, k):
        return (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in (ts * 11)[:k]])

    def raw(px, py, terms):
        return fn(plan._h, px, py, terms, ctypes.c_void_p(key.data_ptr()), ctypes.c_void_p(out.data_ptr()), count, 0,
                  ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    for px, py, terms in ((ptrs(xs, 33), ptrs(ys, 33), 33), (ptrs(xs, 3), ptrs(ys, 3), 0), (None, ptrs(ys, 3), 3),
                          (ptrs(xs, 3), None, 3), (ptrs([xs[0], None, xs[2]], 3), ptrs(ys, 3), 3),
                          (ptrs(xs, 3), ptrs([ys[0], ys[1], None], 3), 3)):
        with g.launch_log() as log:
            assert raw(px, py, terms) != 0
        assert log.kernels == []
    with g.launch_log() as log:
        assert raw(ptrs(xs, 3), ptrs(ys, 3), 3) == 0  # the same raw call, well-formed
    assert log.kernels
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """one stream, a linear capture (no parallel branches), replayed twice with new data"""
    import torch
    n_power, L, K, alpha, count, T = 9, 3, 2, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    xs, ys, key = relin_sum_operands(g, plan, st, np.random.default_rng(0), count, T)
    out = filled(bits, 2 * count * L * n)
    scratch, scratch2 = relin_scratch(plan, count), relin_scratch(plan, count)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.multiply_relinearize_sum(xs, ys, key, out, count, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.multiply_relinearize_sum(xs, ys, key, out, count, True, scratch, stream=s)
    for seed in (1, 2):
        nxs, nys, nkey = relin_sum_operands(g, plan, st, np.random.default_rng(seed), count, T)
        for old, new in zip(xs + ys + [key], nxs + nys + [nkey]):
            old.copy_(new)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize_sum(xs, ys, key, eager, count, True, scratch2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed
        assert torch.equal(eager, composition_relin_sum(g, plan, st, xs, ys, key, count, True)), seed


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_multiply_relin_sum.cpp, compiled here against include/ and libgpuntt.so: three pairs of
    ciphertexts multiplied and summed, compared with the composition"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_multiply_relin_sum")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_multiply_relin_sum.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
