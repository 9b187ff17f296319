"""KeySwitchPlan.linear_transform_bsgs on the MI355X (include/gpuntt/rns/key_switch.cuh): the double-hoisted
baby-step/giant-step linear transform.  Every comparison is torch.equal against the definition --
bsgs_utils.composition_bsgs, built from the calls that existed before -- on the same device data."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bsgs_utils import bsgs_elements, bsgs_operands, bsgs_scratch, composition_bsgs, with_absent
from hoisted_sum_utils import composition_sum, sum_scratch
from hoisted_utils import device_words, filled, make_plan, ring
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


def placed(keys, elts, at):
    """the key list with None at `at` (at == len(keys): every step keeps its key) and the elements with 1 there"""
    if at >= len(keys):
        return list(keys), list(elts)
    return ([None if i == at else k for i, k in enumerate(keys)], [1 if i == at else e for i, e in enumerate(elts)])


def check_against_the_composition(g, plan, st, rng, combos, km_moduli=None, key_limbs=None, offset=0, rescale=False):
    """per (n1, n2, count): all four of {c0 / null} x {output_ntt}; one null baby key and one null giant key at element
    1, at a position that moves between the four (one of them past the end: no null key on that axis), an absent
    weight in every row but never a whole row; the inputs unmodified afterwards"""
    import torch
    bits, n = plan.bits, 1 << plan.n_power
    keep_limbs = plan.kept_count if rescale else plan.q_count
    call = plan.linear_transform_bsgs_rescale if rescale else plan.linear_transform_bsgs
    for n1, n2, count in combos:
        a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, plan, st, rng, count, n1, n2, km_moduli, offset)
        flat = [w for row in weights for w in row]
        keep = [t.clone() for t in (a, c0, c1, *bkeys, *gkeys, *flat)]
        scratch = bsgs_scratch(plan, count, n1, n2)
        for i, (with_c0, output_ntt) in enumerate(itertools.product((False, True), (False, True))):
            bk, be = placed(bkeys, bsgs_elements(g, plan.n_power, n1), i % (n1 + 1))
            gk, ge = placed(gkeys, bsgs_elements(g, plan.n_power, n2), (i + 1) % (n2 + 1))
            w = with_absent(weights, i)
            z0 = c0 if with_c0 else None
            want = composition_bsgs(g, plan, st, a, z0, c1, bk, be, gk, ge, w, count, output_ntt, key_limbs, rescale)
            out = filled(bits, 2 * count * keep_limbs * n, offset)
            call(a, z0, c1, bk, be, gk, ge, w, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (n1, n2, count, with_c0, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((a, c0, c1, *bkeys, *gkeys, *flat), keep)), "an input was modified"


COMBOS = [(1, 1, 1), (3, 2, 3), (1, 3, 1), (4, 1, 3)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 6, 7, 9])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_with_chunks_of_64_slots(g, chunk6, bits, n_power, L, K, alpha, widths=None):
    """sub-chunk rings, one chunk exactly, then 2 and 8 chunks: the source chunk differs per giant step, which is where
    a stale LDS tile or a missing barrier shows"""
    M = L + K
    st = ring(g, bits, n_power, widths=widths).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert g.keyswitch_hoist_sum_chunk(bits, plan.digits, n_power) == min(6, n_power)
    check_against_the_composition(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COMBOS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [6, 7])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_chunks_of_64_slots_on_the_widest_primes(g, chunk6, bits, n_power, L, K, alpha):
    """primes of 62/61 and 30/29 bits (hoisted_utils.WIDE_WIDTHS): 2 q passes 2^(W-1) -- the addition of the v term and
    the carries of the across-g accumulator"""
    test_every_output_word_with_chunks_of_64_slots(g, chunk6, bits, n_power, L, K, alpha, "wide")


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("widths", [None, "wide"])
def test_every_output_word_with_the_automatic_chunk(g, bits, widths):
    n_power, L, K, alpha = 12, 3, 2, 2
    st = ring(g, bits, n_power, widths=widths).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert n_power - g.keyswitch_hoist_sum_chunk(bits, plan.digits, n_power) >= 1  # at least 2 chunks per polynomial
    check_against_the_composition(g, plan, st, np.random.default_rng(L + bits), [(3, 2, 2)])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n1,n2", [(16, 16), (64, 4), (4, 64)])
def test_the_limits_run(g, chunk6, bits, n1, n2):
    n_power, L, K, alpha = 5, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(n1 + bits), [(n1, n2, 1)])


# bsgs_weighted_sum's launch shape by n1: (V words per lane, lanes per workgroup) for u64 and for u32, every base pointer
# 16-byte aligned, on a ring long enough that N decides nothing.  Written out from host::bsgs_sum_shape with its 32 KiB
# LDS budget (n1 * lanes * V * word bytes may not pass it; V falls to one word once 64 lanes of n1 groups do): a change of
# the rule is a conscious edit here
SUM_SHAPES = {8: ((2, 256), (4, 256)), 9: ((2, 128), (4, 128)), 16: ((2, 128), (4, 128)), 17: ((2, 64), (4, 64)),
              32: ((2, 64), (4, 64)), 33: ((1, 64), (1, 128)), 64: ((1, 64), (1, 128))}
SUM_SHAPES_OFF_ALIGNMENT = {17: ((1, 128), (1, 256))}  # a weight one word off 16 bytes: one word per lane


def sum_shape_case(g, bits, n1, table, offset):
    """N = 2^11: the smallest ring at which every shape of the tables has at least two tiles per polynomial (256 lanes
    x 4 words of u32 = 1024 columns) and the N rule never decides; n2 = 2, count = 1"""
    n_power, L, K, alpha = 11, 3, 2, 2
    V, nt = table[n1][0 if bits == 64 else 1]
    assert g.bsgs_sum_shape(bits, n1, n_power, offset == 0) == (V, nt)
    assert (1 << n_power) // (V * nt) >= 2 and n1 * nt * V * (bits // 8) <= 32768
    if n1 == 64:
        assert n1 * nt * V * (bits // 8) == 32768  # the dynamic LDS at the whole budget
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(n1 + bits), [(n1, 2, 1)], offset=offset)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n1", sorted(SUM_SHAPES))
def test_every_launch_shape_of_the_weighted_sum(g, bits, n1):
    """256, 128 and 64 lanes with a 16-byte group per lane, the 64 lanes the LDS budget forces, one word per lane
    because n1 > 32, and n1 = 64 with 32 KiB of dynamic LDS: each asserted through the library's own rule, then run with
    more than one tile per polynomial -- a wrong LDS size or [b][lane] stride only shows on the hardware"""
    sum_shape_case(g, bits, n1, SUM_SHAPES, 0)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_launch_shape_with_base_pointers_off_alignment(g, bits):
    """n1 = 17 with a, c0, c1, the keys, the weights and out one word off 16 bytes: one word per lane, and more lanes
    than the aligned call takes"""
    sum_shape_case(g, bits, 17, SUM_SHAPES_OFF_ALIGNMENT, 1)


def test_the_launch_shape_on_a_ring_shorter_than_a_group(g):
    """N = 2 is shorter than the four words of a u32 group: one word per lane, 64 lanes (n_power = 1 is run against the
    composition by test_every_output_word_with_chunks_of_64_slots); u64's group of two still fits"""
    for n1 in (1, 3, 4, 64):
        assert g.bsgs_sum_shape(32, n1, 1, True) == (1, 64)
    assert g.bsgs_sum_shape(64, 3, 1, True) == (2, 64)
    for bad in ((16, 3, 5), (64, 0, 5), (64, 65, 5), (64, 3, 0), (64, 3, 29)):
        with pytest.raises(ValueError):
            g.bsgs_sum_shape(*bad, True)


@pytest.mark.parametrize("bits", [64, 32])
def test_beyond_the_limits_is_refused(g, bits):
    n_power, L, K, alpha = 5, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, plan, st, np.random.default_rng(1), 1, 1, 1)
    out = filled(bits, 2 * L << n_power)
    scratch = bsgs_scratch(plan, 1, 16, 16)
    for n1, n2 in ((257, 1), (1, 257), (65, 1), (1, 65), (64, 5), (1, 0), (0, 1)):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                plan.linear_transform_bsgs(a, c0, c1, bkeys * n1, [1] * n1, gkeys * n2, [1] * n2,
                                           [weights[0] * n1] * n2, out, 1, False, scratch)
            with pytest.raises(ValueError):
                plan.bsgs_scratch_bytes(1, n1, n2)
        assert log.kernels == []


@pytest.mark.parametrize("bits", [64, 32])
def test_many_digits_force_a_small_chunk(g, bits):
    """(L, K, alpha) = (20, 2, 1): D = 20, 21 rows of LDS per chunk slot -- 128 slots for u64"""
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert plan.digits == 20 and g.keyswitch_hoist_sum_chunk(bits, 20, n_power) == (7 if bits == 64 else 8)
    check_against_the_composition(g, plan, st, np.random.default_rng(20 + bits), [(3, 2, 2)])


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, chunk6, bits):
    """a plan built with X_N_minus: elements reduced mod N, the cyclic slot order"""
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, poly=g.X_N_minus).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(6 + bits), [(3, 2, 3)])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_keys_in_place(g, bits):
    """L = 4 of keys built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_against_the_composition(g, plan, st, np.random.default_rng(bits), [(3, 2, 3)], km_moduli=full.moduli,
                                  key_limbs=limbs)


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """a, c0, c1, the keys, the weights and out one word off 16-byte alignment (the scratch has to be 256-byte aligned)"""
    n_power, L, K, alpha = 7, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, _, c1, _, _, weights = bsgs_operands(g, plan, st, np.random.default_rng(1), 1, 1, 1, offset=1)
    assert a.data_ptr() % 16 and c1.data_ptr() % 16 and weights[0][0].data_ptr() % 16
    check_against_the_composition(g, plan, st, np.random.default_rng(9 + bits), [(3, 2, 3)], offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_degenerate_call_is_rotate_hoisted_sum(g, bits):
    """n2 = 1, a null giant key, every baby key and every weight present: exactly rotate_hoisted_sum's words"""
    import torch
    n_power, L, K, alpha, n1, count = 7, 3, 2, 2, 5, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, c1, bkeys, _, weights = bsgs_operands(g, plan, st, np.random.default_rng(bits), count, n1, 1)
    belts = bsgs_elements(g, n_power, n1, 3)  # the identity among them, with its key
    for with_c0, output_ntt in itertools.product((False, True), (False, True)):
        z0 = c0 if with_c0 else None
        want = filled(bits, 2 * count * L * n)
        plan.rotate_hoisted_sum(a, z0, bkeys, belts, weights[0], want, count, output_ntt, sum_scratch(plan, count))
        out = filled(bits, 2 * count * L * n)
        plan.linear_transform_bsgs(a, z0, None, bkeys, belts, [None], [1], weights, out, count, output_ntt,
                                   bsgs_scratch(plan, count, n1, 1))
        torch.cuda.synchronize()
        assert torch.equal(out, want), (with_c0, output_ntt)
        assert torch.equal(want, composition_sum(g, plan, st, a, z0, bkeys, belts, weights[0], count, output_ntt))


@pytest.mark.parametrize("bits,R", [(64, 1), (32, 2)])
def test_rescale(g, chunk6, bits, R):
    n_power, L, K, alpha = 7, 4, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits, rescale_limbs=R)
    check_against_the_composition(g, plan, st, np.random.default_rng(R + bits), [(3, 2, 2)], rescale=True)
    bare = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, bare, st, np.random.default_rng(1), 1, 1, 1)
    with g.launch_log() as log:
        with pytest.raises(ValueError):
            bare.linear_transform_bsgs_rescale(a, c0, c1, bkeys, [1], gkeys, [1], weights, filled(bits, 2 * L << n_power),
                                               1, False, bsgs_scratch(bare, 1, 1, 1))
    assert log.kernels == []


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and the scratch inside larger sentinel-filled buffers, the scratch exactly bsgs_scratch_bytes long"""
    import torch
    n_power, L, K, alpha, n1, n2, count = 7, 3, 2, 2, 3, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, plan, st, np.random.default_rng(bits), count, n1, n2)
    bk, be = placed(bkeys, bsgs_elements(g, n_power, n1), 1)
    gk, ge = placed(gkeys, bsgs_elements(g, n_power, n2), 0)
    w = with_absent(weights, 1)
    flat = [t for row in weights for t in row]
    keep = [t.clone() for t in (a, c0, c1, *bkeys, *gkeys, *flat)]
    want = composition_bsgs(g, plan, st, a, c0, c1, bk, be, gk, ge, w, count, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = plan.bsgs_scratch_bytes(count, n1, n2)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    plan.linear_transform_bsgs(a, c0, c1, bk, be, gk, ge, w, big_out[pad:pad + words_out], count, True,
                               big_scratch[256:256 + sbytes])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())
    assert all(torch.equal(t, k) for t, k in zip((a, c0, c1, *bkeys, *gkeys, *flat), keep)), "an input was modified"


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha = 64, 9, 6, 2, 2
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    mods = [c.prm.modulus for c in full.cases[:M]]
    N1, N2, C = 3, 2, 3
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, plan, st, np.random.default_rng(5), C, N1, N2)
    out = filled(bits, 2 * C * L * n)
    sbytes = plan.bsgs_scratch_bytes(C, N1, N2)
    big = torch.zeros(sbytes, dtype=torch.uint8, device="cuda:0")
    scratch = big[:sbytes]
    assert scratch.data_ptr() % 256 == 0
    lone = {}

    def ntt_stage(table, kind, mc, batch):
        """the launches of a stand-alone NTTPlan over the first mc moduli for `batch` polynomials"""
        if (kind, mc, batch) not in lone:
            alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
            buf = torch.zeros(batch * n, dtype=torch.int64, device="cuda:0")
            with g.launch_log() as log:
                alone.execute(buf, buf, batch)
            assert log.kernels
            lone[(kind, mc, batch)] = log.kernels
        return lone[(kind, mc, batch)]

    own = {"inner_product_galois", "bsgs_scale_input", "bsgs_weighted_sum", "base_convert", "ks_mod_up",
           "inner_product_galois_giant"}
    skeleton = {}
    for (n1, n2), count in itertools.product(((1, 1), (3, 2)), (1, 3)):
        for null_b, null_g in ((n1, n2), (0, n2), (n1, 0), (0, 0)):
            bk, be = placed(bkeys[:n1], bsgs_elements(g, n_power, n1), null_b)
            gk, ge = placed(gkeys[:n2], bsgs_elements(g, n_power, n2), null_g)
            w = [row[:n1] for row in weights[:n2]]
            n1k, n2k = sum(k is not None for k in bk), sum(k is not None for k in gk)
            before = torch.cuda.memory_allocated()
            for with_c0, output_ntt in itertools.product((False, True), (False, True)):
                with g.launch_log() as log:
                    plan.linear_transform_bsgs(a, c0 if with_c0 else None, c1, bk, be, gk, ge, w, out, count,
                                               output_ntt, scratch)
                want = (["inner_product_galois"] if n1k else []) + (["bsgs_scale_input"] if n1k < n1 else []) + \
                    ["bsgs_weighted_sum"]
                if n2k:
                    want += ntt_stage(st["inv"], g.INVERSE, M, n2k * count * M) + ["base_convert", "ks_mod_up"] + \
                        ntt_stage(st["fwd"], g.FORWARD, M, D * n2k * count * M)
                want += ["inner_product_galois_giant"] + ntt_stage(st["inv"], g.INVERSE, M, 2 * count * M) + \
                    ["base_convert"] + (ntt_stage(st["fwd"], g.FORWARD, L, 2 * count * L) if output_ntt else [])
                assert log.kernels == want, (log.kernels, want)
                # the call's own kernels do not depend on count, n1 or n2 -- only on whether a stage is there at all
                mine = [k for k in log.kernels if k in own]
                assert skeleton.setdefault((n1k > 0, n1k < n1, n2k > 0, output_ntt), mine) == mine
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == before
    n1, n2, count = N1, N2, C
    be, ge = bsgs_elements(g, n_power, n1), bsgs_elements(g, n_power, n2)
    with g.launch_log() as log:
        plan.linear_transform_bsgs(a, c0, c1, bkeys, be, gkeys, ge, weights, out, 0, True, scratch)
    assert log.kernels == []
    tail = scratch.view(torch.int64)
    off = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    ws = weights

    def call(a_=a, c0_=c0, c1_=c1, bk=bkeys, be_=be, gk=gkeys, ge_=ge, w=ws, out_=out, count_=count, scratch_=scratch,
             plan_=plan):
        return lambda: plan_.linear_transform_bsgs(a_, c0_, c1_, bk, be_, gk, ge_, w, out_, count_, False, scratch_)
    no_row = [ws[0], [None] * n1]
    refused = [call(count_=-1), call(count_=1 << 24),                                      # beyond every buffer and limit
               call(be_=be[:2] + [2]), call(be_=be[:2] + [2 << n_power]),                 # an even element (once reduced)
               call(ge_=[2, ge[1]]),
               call(bk=[None] + bkeys[1:]), call(gk=[None] + gkeys[1:]),                  # a null key at an element != 1
               call(c1_=None, bk=[None] + bkeys[1:], be_=[1] + be[1:]),                   # a null baby key needs c1
               call(w=None), call(w=no_row),                                              # no array; a row without a weight
               call(a_=None), call(out_=None), call(scratch_=None),
               call(bk=None), call(be_=None), call(gk=None), call(ge_=None),
               call(bk=bkeys[:2]), call(gk=gkeys[:1]), call(w=ws[:1]), call(w=[ws[0], ws[1][:2]]),
               call(scratch_=bsgs_scratch(plan, count, n1, n2, short=1)),
               call(scratch_=off[8:]),                                                    # not 256-byte aligned
               call(a_=a[1:]), call(c0_=c0[1:]), call(c1_=c1[1:]), call(out_=out[1:]),     # too small
               call(bk=bkeys[:2] + [bkeys[2][1:]]), call(gk=[gkeys[0], gkeys[1][1:]]),
               call(w=[ws[0], ws[1][:2] + [ws[1][2][1:]]]),
               call(a_=a.to(torch.int32)),
               # out or the scratch over a, c0, c1, a key, a weight or each other
               call(a_=tail[:a.numel()]), call(c0_=tail[-c0.numel():]), call(c1_=tail[-c1.numel():]),
               call(bk=bkeys[:2] + [tail[:bkeys[0].numel()]]), call(gk=[gkeys[0], tail[:gkeys[0].numel()]]),
               call(w=[ws[0], ws[1][:2] + [tail[-ws[0][0].numel():]]]),
               call(out_=tail[-out.numel():]),
               call(c0_=out[-c0.numel():]), call(c1_=out[-c1.numel():]),
               call(w=[[out[:ws[0][0].numel()]] + ws[0][1:], ws[1]]),
               call(plan_=bare)]                                                          # no transforms
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """one stream, a linear capture (no parallel branches), replayed twice into a re-poisoned out"""
    import torch
    n_power, L, K, alpha, n1, n2, count = 9, 3, 2, 2, 3, 2, 2
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, plan, st, np.random.default_rng(0), count, n1, n2)
    bk, be = placed(bkeys, bsgs_elements(g, n_power, n1), 0)
    gk, ge = placed(gkeys, bsgs_elements(g, n_power, n2), 0)
    w = with_absent(weights, 1)
    out = filled(bits, 2 * count * L * n)
    scratch, scratch2 = bsgs_scratch(plan, count, n1, n2), bsgs_scratch(plan, count, n1, n2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.linear_transform_bsgs(a, c0, c1, bk, be, gk, ge, w, out, count, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.linear_transform_bsgs(a, c0, c1, bk, be, gk, ge, w, out, count, True, scratch, stream=s)
    eager = filled(bits, 2 * count * L * n)
    plan.linear_transform_bsgs(a, c0, c1, bk, be, gk, ge, w, eager, count, True, scratch2)
    torch.cuda.synchronize()
    assert torch.equal(eager, composition_bsgs(g, plan, st, a, c0, c1, bk, be, gk, ge, w, count, True))
    for _ in range(2):
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_computes_the_matrix_product(g, bits):
    """The noiseless instance of test_gpu_hoisted_sum.test_it_really_computes_a_linear_transform with n1 = n2 = 2: c0 +
    c1 s = msg (mod Q); baby steps {identity with a null key, rotation by 1}, giant steps {identity with a null key,
    rotation by 2}, the two real keys noiseless, key_k[d] = (-a_d s + P g_d sigma_k(s), a_d); the four diagonals small
    signed integers in [-50, 50].

    Derivation of the bound.  As that test derives, every baby accumulator satisfies u_b[0] + u_b[1] s = P sigma_b(msg)
    (mod P Q) exactly (the null-key step holds P c0 and P c1 themselves), and the weighted sums are taken in the ring mod
    P Q word for word, so V_g = (V_g0, V_g1) has V_g0 + V_g1 s = P X_g (mod P Q), X_g = sum_b pt_{g,b} sigma_b(msg).
    A giant step without a key adds V_g itself: no error.  A giant step WITH a key takes t_g = mod_down(V_g1) =
    (V_g1 - conv_g) / P, conv_g the residue of V_g1 mod P that mod_down removes, |conv_g| <= P (1/2 + 3 K / 2^W).  Its
    digits, permuted, are digits of sigma_g(t_g), and the noiseless key gives accumulators (A_0, A_1) with
    A_0 + A_1 s = P sigma_g(t_g) sigma_g(s) (mod P Q) exactly; adding sigma_g(V_g0) to A_0 (multiplier 1: V_g0 is
    already at scale P) gives sigma_g(V_g0 + P t_g s) = sigma_g(V_g0 + V_g1 s - conv_g s) = P sigma_g(X_g) -
    sigma_g(conv_g s).  So before the final ModDown the combination is P sum_g sigma_g(X_g) minus, per keyed giant step,
    sigma_g(conv_g s) of infinity norm at most |conv_g| h, h = |s|_1: at most h / 2 + 1 after the division by P.  The
    single final ModDown adds (1 + h) / 2 + 1 as in that test.  Total: (1 + h) / 2 + 1 + n2k (h / 2 + 1), n2k = 1."""
    import torch
    n_power, L, K, alpha = 5, 3, 2, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    full, qs, ps = st["moduli"], st["moduli"][:L], st["moduli"][L:]
    Q, P = math.prod(qs), math.prod(ps)
    plan = make_plan(g, st, L, alpha, n_power, bits)
    rng = np.random.default_rng(29 + bits)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    h = int(sum(abs(v) for v in s))
    k1, k2 = g.galois_element_for_rotation(1, n_power), g.galois_element_for_rotation(2, n_power)

    def sigma(x, k):  # a(X) -> a(X^k) in Z[X] / (X^N + 1)
        out = np.zeros(n, dtype=object)
        for i in range(n):
            e = (i * k) % (2 * n)
            out[e % n] += x[i] if e < n else -x[i]
        return out

    parts = partition(L, alpha)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)

    def switching_key(k):
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
        return d_key

    def ntt_form(x, moduli):
        d = device_words(g, words(g, np.array([x % q for q in moduli], dtype=object), bits))
        g.GPU_NTT_Inplace(d, st["fwd"], st["mods"], cfg_f, len(moduli), len(moduli))
        return d

    pts = [[np.array([int(v) for v in rng.integers(-50, 51, size=n)], dtype=object) for _ in range(2)] for _ in range(2)]
    weights = [[ntt_form(pt, full) for pt in row] for row in pts]
    c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
    msg = np.array([int(v) for v in rng.integers(-1000, 1000, size=n)], dtype=object)
    c0 = (msg - negacyclic(c1, s)) % Q
    d_c1 = device_words(g, words(g, np.array([c1 % q for q in qs], dtype=object), bits))
    a = filled(bits, plan.digits * M * n)
    plan.decompose(d_c1, a, 1, False, None)
    out = filled(bits, 2 * L * n)
    plan.linear_transform_bsgs(a, ntt_form(c0, qs), ntt_form(c1, qs), [None, switching_key(k1)], [1, k1],
                               [None, switching_key(k2)], [1, k2], weights, out, 1, False, bsgs_scratch(plan, 1, 2, 2))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    bound = (1 + h) / 2 + 1 + 1 * (h / 2 + 1)
    want = sum(sigma(sum(negacyclic(pts[gi][b], sigma(msg, kb)) for b, kb in enumerate((1, k1))), kg)
               for gi, kg in enumerate((1, k2)))
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    err = [abs(int(v)) for v in centre((value - want) % Q, Q)]
    print("largest error %d, bound %.1f" % (max(err), bound))
    assert max(err) <= bound, (max(err), bound)


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_linear_transform.cpp, compiled here against include/ and libgpuntt.so: a 3 x 2 baby-step/
    giant-step transform of one ciphertext from one decompose, compared with the composition"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_linear_transform")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_linear_transform.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
