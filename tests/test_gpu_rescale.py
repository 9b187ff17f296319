"""KeySwitchPlan's rescaling calls on the MI355X (include/gpuntt/rns/key_switch.cuh, "Rescaling"): mod_down_rescale,
rescale in both forms and the three *_rescale pipeline calls.  Every comparison is torch.equal against a composition of
the calls that existed before (rescale_utils) on the same device data, or array_equal against the host references and
rescale_exact's Python integers."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hoisted_exact import exact_u, exact_weighted_sum, host_cases, transform
from hoisted_sum_utils import make_weights, sum_scratch, with_nones
from hoisted_utils import (WIDE_WIDTHS, any_words, canonical_key, device_words, elements_for, filled, make_plan, ring)
from innerprod_utils import from_words
from relin_sum_utils import relin_sum_operands
from relin_utils import composition_relin, relin_operands, relin_scratch
from rescale_exact import exact_multiply_relinearize_rescale, finish_rescale
from rescale_utils import (composition_relin_rescale, composition_rescale, composition_sum_rescale, dense_divide)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 2, 1), (6, 2, 2, 2), (4, 1, 2, 3)]  # (L, K, alpha, R); the last leaves one kept limb
RINGS = [1, 2, 5, 9, 12]  # N = 2 at u32: the one-word loader; 2^12: several column tiles per polynomial
COUNTS = (1, 3, 5)        # RB = 1; 2 with a ragged tail; 4 with a ragged tail


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def plan_for(g, bits, n_power, L, K, alpha, R, widths=None, poly=None, **kw):
    st = ring(g, bits, n_power, poly=poly, widths=widths).sub(list(range(L + K)))
    return st, make_plan(g, st, L, alpha, n_power, bits, rescale_limbs=R, **kw)


def rescale_scratch(plan, stacks):
    import torch
    return torch.zeros(max(256, plan.rescale_scratch_bytes(stacks)), dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", RINGS)
@pytest.mark.parametrize("L,K,alpha,R", SHAPES)
def test_mod_down_rescale_and_rescale_in_coefficient_form(g, bits, n_power, L, K, alpha, R):
    """every output word against BaseConvPlan.convert_and_divide on gathered dense copies of the same device data and
    against the host references; exactly one kernel each; the inputs unmodified"""
    import torch
    M, n, stacks = L + K, 1 << n_power, 3
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    assert plan.rescale_limbs == R and plan.kept_count == L - R
    rng = np.random.default_rng(bits + n_power + 10 * L)
    dt = g.np_dtype(bits)
    for limbs, moduli, call, ref in (
            (M, st["moduli"], lambda x, o: plan.mod_down_rescale(x, o, stacks),
             lambda h, o: g.keyswitch_reference_mod_down_rescale(st["moduli"][:L], st["moduli"][L:], R, h, o, n_power,
                                                                 stacks, bits=bits)),
            (L, st["moduli"][:L], lambda x, o: plan.rescale(x, o, stacks, False),
             lambda h, o: g.keyswitch_reference_rescale(st["moduli"][:L], R, h, o, n_power, stacks, bits=bits))):
        hx = any_words(g, rng, bits, stacks * limbs * n, moduli)
        x = device_words(g, hx)
        keep = x.clone()
        out = filled(bits, stacks * (L - R) * n)
        with g.launch_log() as log:
            call(x, out)
        torch.cuda.synchronize()
        assert log.kernels == ["base_convert"], log.kernels
        assert torch.equal(out, dense_divide(g, moduli, L - R, x, stacks, n_power, bits)), limbs
        want = np.zeros(stacks * (L - R) * n, dtype=dt)
        ref(hx, want)
        assert np.array_equal(g.to_host(out), want), limbs
        assert torch.equal(x, keep), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", RINGS)
@pytest.mark.parametrize("L,K,alpha,R", SHAPES)
@pytest.mark.parametrize("offset", [0, 1])
def test_rescale_in_ntt_form(g, bits, n_power, L, K, alpha, R, offset):
    """against GPU_INTT -> gathers -> convert_and_divide -> GPU_NTT on the sub-ring, every output word; x holds any
    words (the composition reads them modulo q on the host first); x and out one word off 16-byte alignment too"""
    import torch
    n, stacks = 1 << n_power, 3
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    qs = st["moduli"][:L]
    rng = np.random.default_rng(bits + n_power + 10 * L + offset)
    hx = any_words(g, rng, bits, stacks * L * n, qs)
    x = device_words(g, hx, offset)
    keep = x.clone()
    red = hx.reshape(stacks, L, n) % np.array(qs, dtype=g.np_dtype(bits))[None, :, None]
    want = composition_rescale(g, plan, st, g.to_device(np.ascontiguousarray(red.reshape(-1))), stacks, True)
    out = filled(bits, stacks * (L - R) * n, offset)
    plan.rescale(x, out, stacks, True, rescale_scratch(plan, stacks))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(x, keep), "an input was modified"


def check_relin(g, plan, st, rng, counts, terms_list=(1,), key_limbs=None, km_moduli=None):
    import torch
    bits, n, Lk = plan.bits, 1 << plan.n_power, plan.kept_count
    for count, terms in itertools.product(counts, terms_list):
        xs, ys, key = relin_sum_operands(g, plan, st, rng, count, terms, km_moduli)
        keep = [t.clone() for t in (*xs, *ys, key)]
        scratch = relin_scratch(plan, count)
        for output_ntt in (False, True):
            want = composition_relin_rescale(g, plan, st, xs, ys, key, count, output_ntt, key_limbs)
            out = filled(bits, 2 * count * Lk * n)
            plan.multiply_relinearize_sum_rescale(xs, ys, key, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), ("sum", count, terms, output_ntt)
            if terms == 1:  # with one pair the summed call returns multiply_relinearize_rescale's words
                one = filled(bits, 2 * count * Lk * n)
                plan.multiply_relinearize_rescale(xs[0], ys[0], key, one, count, output_ntt, scratch)
                torch.cuda.synchronize()
                assert torch.equal(one, want), ("one", count, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((*xs, *ys, key), keep)), "an input was modified"


def hoisted_operands(g, plan, st, rng, count, G):
    bits, n = plan.bits, 1 << plan.n_power
    L, M, D = plan.q_count, plan.mod_count, plan.digits
    a = device_words(g, any_words(g, rng, bits, D * count * M * n, st["moduli"]))
    c0 = device_words(g, any_words(g, rng, bits, count * L * n, st["moduli"][:L]))
    keys = [device_words(g, canonical_key(g, rng, bits, st["moduli"], D * 2 * M, n)) for _ in range(G)]
    return a, c0, keys, make_weights(g, plan, st, rng, G)


def check_hoisted_sum(g, plan, st, rng, combos):
    import torch
    bits, n, Lk = plan.bits, 1 << plan.n_power, plan.kept_count
    for G, count in combos:
        elts = elements_for(g, plan.n_power, G)
        a, c0, keys, weights = hoisted_operands(g, plan, st, rng, count, G)
        keep = [t.clone() for t in (a, c0, *keys, *weights)]
        scratch = sum_scratch(plan, count)
        # (c0, weights, output_ntt): without and with weights, without and with c0, both output forms
        for with_c0, w, output_ntt in ((False, None, False), (True, with_nones(weights, 1), True),
                                       (True, None, True), (False, list(weights), False)):
            want = composition_sum_rescale(g, plan, st, a, c0 if with_c0 else None, keys, elts, w, count, output_ntt)
            out = filled(bits, 2 * count * Lk * n)
            plan.rotate_hoisted_sum_rescale(a, c0 if with_c0 else None, keys, elts, w, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (G, count, with_c0, w is None, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((a, c0, *keys, *weights), keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", RINGS)
@pytest.mark.parametrize("L,K,alpha,R", SHAPES)
def test_multiply_relinearize_rescale_every_output_word(g, bits, n_power, L, K, alpha, R):
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    check_relin(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COUNTS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [2, 9])
@pytest.mark.parametrize("L,K,alpha,R", SHAPES)
def test_multiply_relinearize_sum_rescale_three_terms(g, bits, n_power, L, K, alpha, R):
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    check_relin(g, plan, st, np.random.default_rng(n_power + L + bits), (3,), terms_list=(3,))


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", RINGS)
@pytest.mark.parametrize("L,K,alpha,R", SHAPES)
def test_rotate_hoisted_sum_rescale_every_output_word(g, bits, n_power, L, K, alpha, R):
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    check_hoisted_sum(g, plan, st, np.random.default_rng(7 * n_power + L + bits), [(1, 1), (5, 3)])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [6, 12])
@pytest.mark.parametrize("widths", ["wide", "spread"])
def test_on_the_widest_primes(g, bits, n_power, widths):
    """primes of 62/61 and 30/29 bits, and primes spread over the eighth below 2^(W-2)"""
    import torch
    L, K, alpha, R, stacks = 3, 2, 2, 1, 2
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R, widths=widths)
    rng = np.random.default_rng(n_power + bits)
    check_relin(g, plan, st, rng, (3,), terms_list=(1, 3))
    check_hoisted_sum(g, plan, st, rng, [(5, 1)])
    qs = st["moduli"][:L]
    hx = any_words(g, rng, bits, stacks * L * n, qs) % np.tile(np.repeat(np.array(qs, dtype=g.np_dtype(bits)), n), stacks)
    x = g.to_device(hx)
    out = filled(bits, stacks * (L - R) * n)
    plan.rescale(x, out, stacks, True, rescale_scratch(plan, stacks))
    torch.cuda.synchronize()
    assert torch.equal(out, composition_rescale(g, plan, st, x, stacks, True))


@pytest.mark.parametrize("bits", [64, 32])
def test_against_exact_integers_on_the_widest_primes(g, bits):
    """rescale_exact and hoisted_exact: no GPU call and none of the library's arithmetic"""
    import torch
    n_power, L, K, alpha, R, count, G = 5, 3, 2, 2, 1, 3, 3
    M, n = L + K, 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R, widths="wide")
    cases = host_cases(bits, n_power, WIDE_WIDTHS[bits], M)
    assert [c.q for c in cases] == st["moduli"]
    rng = np.random.default_rng(bits)
    x, y, key = relin_operands(g, plan, st, rng, count)
    hx, hy = (from_words(g.to_host(t), (2, count, L, n)) for t in (x, y))
    hkey = from_words(g.to_host(key), (plan.digits, 2, M, n))
    a, c0, keys, weights = hoisted_operands(g, plan, st, rng, count, G)
    elts = elements_for(g, n_power, G)
    ha, hc0 = from_words(g.to_host(a), (plan.digits, count, M, n)), from_words(g.to_host(c0), (count, L, n))
    hkeys = [from_words(g.to_host(k), (plan.digits, 2, M, n)) for k in keys]
    hw = [from_words(g.to_host(w), (M, n)) for w in weights]
    acc = exact_weighted_sum(st["moduli"], exact_u(g, st["moduli"], L, n_power, st["poly"], ha, hc0, hkeys, elts), hw)
    stack = transform(cases, acc.reshape(-1, M, n), True).reshape(acc.shape)
    for output_ntt in (False, True):
        out = filled(bits, 2 * count * (L - R) * n)
        plan.multiply_relinearize_rescale(x, y, key, out, count, output_ntt, relin_scratch(plan, count))
        torch.cuda.synchronize()
        want = exact_multiply_relinearize_rescale(cases, L, R, alpha, bits, hx, hy, hkey, output_ntt)
        assert np.array_equal(from_words(g.to_host(out), want.shape), want), output_ntt
        plan.rotate_hoisted_sum_rescale(a, c0, keys, elts, weights, out, count, output_ntt, sum_scratch(plan, count))
        torch.cuda.synchronize()
        want = finish_rescale(cases, L, R, stack, bits, output_ntt)
        assert np.array_equal(from_words(g.to_host(out), want.shape), want), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, bits):
    import torch
    n_power, L, K, alpha, R, stacks = 6, 3, 2, 2, 1, 3
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R, poly=g.X_N_minus)
    rng = np.random.default_rng(6 + bits)
    check_relin(g, plan, st, rng, (3,))
    check_hoisted_sum(g, plan, st, rng, [(5, 1)])
    x = device_words(g, canonical_key(g, rng, bits, st["moduli"][:L], stacks * L, n))
    out = filled(bits, stacks * (L - R) * n)
    plan.rescale(x, out, stacks, True, rescale_scratch(plan, stacks))
    torch.cuda.synchronize()
    assert torch.equal(out, composition_rescale(g, plan, st, x, stacks, True))


@pytest.mark.parametrize("bits", [64, 32])
def test_out_over_an_operand(g, bits):
    """out given as x, then as y, each compared with an out-of-place run; out has fewer words than an operand"""
    import torch
    n_power, L, K, alpha, R, count = 9, 3, 2, 2, 1, 3
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(3 + bits), count)
    scratch = relin_scratch(plan, count)
    words_out = 2 * count * (L - R) * n
    for output_ntt in (False, True):
        out = filled(bits, words_out)
        plan.multiply_relinearize_rescale(x, y, key, out, count, output_ntt, scratch)
        xc, yc = x.clone(), y.clone()
        plan.multiply_relinearize_rescale(xc, y, key, xc, count, output_ntt, scratch)
        plan.multiply_relinearize_rescale(x, yc, key, yc, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(xc[:words_out], out) and torch.equal(yc[:words_out], out), output_ntt
        assert torch.equal(xc[words_out:], x[words_out:]) and torch.equal(yc[words_out:], y[words_out:])


@pytest.mark.parametrize("bits", [64, 32])
def test_the_result_chains_into_the_next_level(g, bits):
    """multiply_relinearize_rescale at L = 4, R = 1 writes a ciphertext over 3 limbs; a plan built for L = 3 multiplies it
    again, reading the same full-level key through key_mod_count / key_limbs"""
    import torch
    n_power, alpha, count = 9, 2, 2
    n = 1 << n_power
    full = ring(g, bits, n_power)
    top_limbs = [0, 1, 2, 3, 6, 7]  # of a key built for 6 + 2 limbs
    st4 = full.sub(top_limbs)
    plan4 = make_plan(g, st4, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=top_limbs, rescale_limbs=1)
    low_limbs = [0, 1, 2, 6, 7]
    st3 = full.sub(low_limbs)
    plan3 = make_plan(g, st3, 3, alpha, n_power, bits, key_mod_count=8, key_limbs=low_limbs)
    rng = np.random.default_rng(bits)
    x, y, key = relin_operands(g, plan4, st4, rng, count, km_moduli=full.moduli)
    mid = filled(bits, 2 * count * 3 * n)
    plan4.multiply_relinearize_rescale(x, y, key, mid, count, True, relin_scratch(plan4, count))
    torch.cuda.synchronize()
    assert torch.equal(mid, composition_relin_rescale(g, plan4, st4, [x], [y], key, count, True, top_limbs))
    out = filled(bits, 2 * count * 3 * n)
    plan3.multiply_relinearize(mid, mid, key, out, count, True, relin_scratch(plan3, count))
    torch.cuda.synchronize()
    assert torch.equal(out, composition_relin(g, plan3, st3, mid, mid, key, count, True))


@pytest.mark.parametrize("bits", [64, 32])
def test_a_plan_with_no_rescale_limbs_from_the_new_create_function_is_the_old_plan(g, bits):
    import torch
    n_power, L, K, alpha, count = 7, 3, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    old = make_plan(g, st, L, alpha, n_power, bits)
    new = make_plan(g, st, L, alpha, n_power, bits, rescale_limbs=0, via_rescale_abi=True)
    assert new.rescale_limbs == 0 and old.rescale_limbs == 0
    x, y, key = relin_operands(g, old, st, np.random.default_rng(bits), count)
    scratch = relin_scratch(old, count)
    outs = []
    for plan in (old, new):
        with g.launch_log() as log:
            o1, o2 = filled(bits, 2 * count * L * n), filled(bits, 2 * count * L * n)
            plan.apply(x[:count * L * n], key, o1, count, 2, True, True, scratch)
            plan.multiply_relinearize(x, y, key, o2, count, True, scratch)
        torch.cuda.synchronize()
        outs.append((o1, o2, log.kernels))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    calls = [lambda: new.mod_down_rescale(x, y, 1), lambda: new.rescale(x, y, 1, False),
             lambda: new.rescale(x, y, 1, True, scratch), lambda: new.rescale_scratch_bytes(1),
             lambda: new.multiply_relinearize_rescale(x, y, key, o2, count, True, scratch),
             lambda: new.multiply_relinearize_sum_rescale([x], [y], key, o2, count, True, scratch)]
    for i, f in enumerate(calls):  # every rescale method refuses a plan with R = 0
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha, R = 64, 9, 6, 2, 2, 2
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    rng = np.random.default_rng(5)
    logs = {}
    for stacks in (2, 10):
        x = device_words(g, any_words(g, rng, bits, stacks * L * n, st["moduli"][:L]))
        out = filled(bits, stacks * (L - R) * n)
        scratch = rescale_scratch(plan, stacks)
        torch.cuda.synchronize()
        before, allocs = torch.cuda.memory_allocated(), g.alloc_count()
        with g.launch_log() as log:
            plan.rescale(x, out, stacks, True, scratch)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before and g.alloc_count() == allocs
        logs[stacks] = log.kernels
    assert logs[2] == logs[10] and logs[2][0] == "rescale_gather" and logs[2][-1] == "rescale_sub_scale", logs
    assert logs[2].count("base_convert") == 1
    stacks = 2
    with g.launch_log() as log:
        plan.rescale(x, out, 0, True, scratch)
        plan.rescale(x, out, 0, False)
        plan.mod_down_rescale(x, out, 0)
    assert log.kernels == []
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits, rescale_limbs=R)
    bare.rescale(x, out, stacks, False)  # a plan without transforms: the coefficient form works
    big = torch.zeros(plan.rescale_scratch_bytes(stacks) + 512, dtype=torch.uint8, device="cuda:0")
    words = x.numel()
    refused = [lambda: plan.rescale(None, out, stacks, True, scratch),
               lambda: plan.rescale(x, None, stacks, True, scratch),
               lambda: plan.rescale(x, out, stacks, True, None),                # a null scratch
               lambda: plan.rescale(x, out, stacks, True, big[8:]),             # not 256-byte aligned
               lambda: plan.rescale(x, out, stacks, True, big[:64]),            # too small
               lambda: plan.rescale(x, out, -1, True, scratch),
               lambda: plan.rescale(x, x, stacks, True, scratch),               # out over x
               lambda: plan.rescale(x, x[n:], stacks, False),
               lambda: plan.rescale(x, out, stacks, True, x.view(torch.uint8)),     # the scratch over x
               lambda: plan.rescale(x, out, stacks, True, out.view(torch.uint8)),   # the scratch over out
               lambda: plan.rescale(x[:stacks * L * n - 1], out, stacks, True, scratch),   # too small
               lambda: plan.mod_down_rescale(x, x, 1),
               lambda: plan.mod_down_rescale(x, None, 1),
               lambda: bare.rescale(x, out, stacks, True, scratch),             # no transforms
               lambda: g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits, rescale_limbs=L),
               lambda: g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits, rescale_limbs=-1)]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """multiply_relinearize_rescale and rescale(ntt_form=True), each captured once on one stream (a linear capture, no
    parallel branches) and replayed twice with new data; nothing is allocated by the calls"""
    import torch
    n_power, L, K, alpha, R, count = 9, 3, 2, 2, 1, 2
    n, stacks = 1 << n_power, 2 * 2
    st, plan = plan_for(g, bits, n_power, L, K, alpha, R)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(0), count)
    out = filled(bits, 2 * count * (L - R) * n)
    rout = filled(bits, stacks * (L - R) * n)
    scratch, scratch2 = relin_scratch(plan, count), relin_scratch(plan, count)
    rs, rs2 = rescale_scratch(plan, stacks), rescale_scratch(plan, stacks)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.multiply_relinearize_rescale(x, y, key, out, count, True, scratch, stream=s)
        plan.rescale(x, rout, stacks, True, rs, stream=s)
    s.synchronize()
    allocs = g.alloc_count()
    graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
    with torch.cuda.graph(graphs[0], stream=s):
        plan.multiply_relinearize_rescale(x, y, key, out, count, True, scratch, stream=s)
    with torch.cuda.graph(graphs[1], stream=s):
        plan.rescale(x, rout, stacks, True, rs, stream=s)
    for seed in (1, 2):
        nx, ny, nkey = relin_operands(g, plan, st, np.random.default_rng(seed), count)
        x.copy_(nx), y.copy_(ny), key.copy_(nkey)
        torch.cuda.synchronize()
        graphs[0].replay()
        graphs[1].replay()
        torch.cuda.synchronize()
        eager, reager = filled(bits, out.numel()), filled(bits, rout.numel())
        plan.multiply_relinearize_rescale(x, y, key, eager, count, True, scratch2)
        plan.rescale(x, reager, stacks, True, rs2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(rout, reager), seed
        assert torch.equal(eager, composition_relin_rescale(g, plan, st, [x], [y], key, count, True)), seed
    assert g.alloc_count() == allocs


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_multiply_rescale.cpp, compiled here against include/ and libgpuntt.so: a product rescaled in
    its ModDown and an NTT-form rescale, compared with the host references and with each other; it prints its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_multiply_rescale")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_multiply_rescale.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
