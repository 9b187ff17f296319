"""KeySwitchPlan.mod_down_add, KeySwitchPlan.relinearize (include/gpuntt/rns/key_switch.cuh) and
BfvMultiplyPlan.multiply_relinearize (include/gpuntt/rns/bfv_multiply.cuh) on the MI355X.  Every comparison is torch.equal
against the definition -- relin3_utils' compositions of mod_down, apply, multiply, the transforms and operator_gpu's modular
addition on the same device data -- or array_equal against relin3_exact's Python integers."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bfv_utils import bfv_scratch, operands, reduced
from bfv_utils import make_plan as make_bfv_plan
from hoisted_exact import host_cases
from hoisted_utils import WIDE_WIDTHS, any_words, device_words, filled, make_plan, ring
from innerprod_utils import from_words, words
from keyswitch_utils import centre, crt, negacyclic
from relin3_exact import exact_bfv_multiply_relinearize, exact_definition
from relin3_utils import (bases, composition_bfv, composition_mod_down_add, composition_relinearize, relin3_operands)
from relin_utils import composition_relin, relin_operands, relin_scratch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 3, 5)  # RB = 1; 2 with a ragged tail; 4 with a ragged tail
FORMS = list(itertools.product((False, True), repeat=2))
T = {64: (1 << 40) + 15, 32: 65537}


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


# ---------------------------------------------------------------------------------------------------- mod_down_add
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9, 12])
@pytest.mark.parametrize("L,K", [(3, 2), (6, 2), (5, 3)])
def test_mod_down_add_every_output_word(g, bits, n_power, L, K):
    """(6, 2) and (5, 3) leave a ragged BC_KB block; the output split chosen by the library and forced to 2; the addend of
    any words with 0, q - 1, q and 2^W - 1 planted, separate and exactly out; every base one word off 16-byte alignment"""
    import torch
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], 2, n_power, bits=bits)  # no transforms needed
    rng = np.random.default_rng(bits + 10 * n_power + L)
    try:
        for stacks, split, offset in itertools.product((1, 3), (0, 2), (0, 1)):
            g.set_test_hook("baseconv_ksplit", split)
            x = device_words(g, any_words(g, rng, bits, stacks * M * n, st["moduli"]), offset)
            addend = device_words(g, any_words(g, rng, bits, stacks * L * n, st["moduli"][:L]), offset)
            keep = [x.clone(), addend.clone()]
            want = composition_mod_down_add(g, plan, st, x, addend, stacks)
            out = filled(bits, stacks * L * n, offset)
            with g.launch_log() as log:
                plan.mod_down_add(x, addend, out, stacks)
            torch.cuda.synchronize()
            assert log.kernels == ["mod_down_add"], log.kernels
            assert torch.equal(out, want), (stacks, split, offset)
            assert torch.equal(x, keep[0]) and torch.equal(addend, keep[1]), "an input was modified"
            plan.mod_down_add(x, addend, addend, stacks)  # the addend exactly out
            torch.cuda.synchronize()
            assert torch.equal(addend, want), (stacks, split, offset)
    finally:
        g.set_test_hook("baseconv_ksplit", 0)


# ----------------------------------------------------------------------------------------------------- relinearize
def check_relinearize(g, plan, st, rng, counts, km_moduli=None, offset=0):
    """the contiguous three-component layout and a separate c2; out separate and exactly c01"""
    import torch
    bits, n, L = plan.bits, 1 << plan.n_power, plan.q_count
    for count in counts:
        low = 2 * count * L * n
        scratch = relin_scratch(plan, count)
        for input_ntt, output_ntt in FORMS:
            ct, key = relin3_operands(g, plan, st, rng, count, input_ntt, km_moduli, offset)
            keep = [ct.clone(), key.clone()]
            want = composition_relinearize(g, plan, st, ct[:low], ct[low:], key, count, input_ntt, output_ntt)
            out = filled(bits, low, offset)
            plan.relinearize(ct[:low], ct[low:], key, out, count, input_ntt, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (count, input_ntt, output_ntt)
            assert torch.equal(ct, keep[0]) and torch.equal(key, keep[1]), "an input was modified"
            c2 = device_words(g, g.to_host(ct[low:]), offset)  # a separate top component
            plan.relinearize(ct[:low], c2, key, ct[:low], count, input_ntt, output_ntt, scratch)  # out exactly c01
            torch.cuda.synchronize()
            assert torch.equal(ct[:low], want), (count, input_ntt, output_ntt, "in place")


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9, 12])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_relinearize_every_output_word(g, bits, n_power, L, K, alpha):
    """N = 2 at u32 is below a 16-byte group: the one-word loader; 2^12 has several column tiles per polynomial"""
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_relinearize(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COUNTS)


@pytest.mark.parametrize("bits", [64, 32])
def test_relinearize_on_the_widest_primes(g, bits):
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, widths="wide").sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_relinearize(g, plan, st, np.random.default_rng(n_power + bits), COUNTS)


@pytest.mark.parametrize("bits", [64, 32])
def test_relinearize_on_one_cyclic_ring(g, bits):
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, poly=g.X_N_minus).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_relinearize(g, plan, st, np.random.default_rng(6 + bits), [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_relinearize_twenty_digits(g, bits):
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert plan.digits == 20
    check_relinearize(g, plan, st, np.random.default_rng(20 + bits), [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_key_in_place(g, bits):
    """L = 4 of a key built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_relinearize(g, plan, st, np.random.default_rng(bits), [3], km_moduli=full.moduli)


@pytest.mark.parametrize("bits", [64, 32])
def test_relinearize_base_pointers_one_word_off_alignment(g, bits):
    """c01, c2, the key and out one word off 16-byte alignment (the scratch has to be 256-byte aligned)"""
    n_power, L, K, alpha = 7, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    ct, key = relin3_operands(g, plan, st, np.random.default_rng(1), 1, True, offset=1)
    assert ct.data_ptr() % 16 and key.data_ptr() % 16
    check_relinearize(g, plan, st, np.random.default_rng(9 + bits), COUNTS, offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_relinearize_of_a_tensor_returns_multiply_relinearizes_words(g, bits):
    """(d0, d1, d2) formed by a q-base multiply_accumulate from x and y, reduced: relinearize(input_ntt = true) returns
    the words of multiply_relinearize(x, y)"""
    import torch
    from relin_utils import q_inner_plan
    n_power, L, K, alpha, count = 7, 3, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(bits), count)
    xr, yr = (reduced(g, v, st["moduli"][:L], n, bits).view(2, count, L, n) for v in (x, y))
    inner = q_inner_plan(g, st["moduli"][:L], bits)
    d = filled(bits, 3 * count * L * n).view(3, count, L, n)
    for r in range(count):
        inner.multiply_accumulate(xr[0, r].reshape(-1), yr[0, r].reshape(-1), d[0, r].view(-1), n_power, 1, 1, 1)
        inner.multiply_accumulate(torch.stack((xr[0, r], xr[1, r])).reshape(-1),
                                  torch.stack((yr[1, r], yr[0, r])).reshape(-1), d[1, r].view(-1), n_power, 2, 1, 1)
        inner.multiply_accumulate(xr[1, r].reshape(-1), yr[1, r].reshape(-1), d[2, r].view(-1), n_power, 1, 1, 1)
    d = d.view(-1)
    low = 2 * count * L * n
    scratch = relin_scratch(plan, count)
    for output_ntt in (False, True):
        want, out = filled(bits, low), filled(bits, low)
        plan.multiply_relinearize(x, y, key, want, count, output_ntt, scratch)
        plan.relinearize(d[:low], d[low:], key, out, count, True, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(out, want), output_ntt
        assert torch.equal(out, composition_relin(g, plan, st, x, y, key, count, output_ntt)), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 7])
def test_relinearize_against_exact_integers_on_the_widest_primes(g, bits, n_power):
    """relin3_exact: no GPU call and none of the library's arithmetic"""
    import torch
    L, K, alpha, count = 3, 2, 2, 3
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power, widths="wide").sub(list(range(M)))
    cases = host_cases(bits, n_power, WIDE_WIDTHS[bits], M)
    assert [c.q for c in cases] == st["moduli"]
    plan = make_plan(g, st, L, alpha, n_power, bits)
    scratch = relin_scratch(plan, count)
    low = 2 * count * L * n
    for input_ntt, output_ntt in FORMS:
        ct, key = relin3_operands(g, plan, st, np.random.default_rng(bits + n_power), count, input_ntt)
        h = from_words(g.to_host(ct), (3, count, L, n))
        hkey = from_words(g.to_host(key), (plan.digits, 2, M, n))
        out = filled(bits, low)
        plan.relinearize(ct[:low], ct[low:], key, out, count, input_ntt, output_ntt, scratch)
        torch.cuda.synchronize()
        want = exact_definition(cases, L, alpha, bits, h[:2], h[2], hkey, input_ntt, output_ntt)
        assert np.array_equal(from_words(g.to_host(out), want.shape), want), (input_ntt, output_ntt)


# ------------------------------------------------------------------------- BfvMultiplyPlan.multiply_relinearize
def bfv_plans(g, bits, n_power, L, t=None, widths=None, poly=None):
    t = T[bits] if t is None else t
    full, st_b, st_p, K_b = bases(g, bits, n_power, L, t, poly=poly, widths=widths)
    return full, st_b, st_p, make_bfv_plan(g, st_b, L, t, n_power, bits), make_plan(g, st_p, L, 2, n_power, bits)


def bfv_key(g, rng, ks, st_p, offset=0):
    from hoisted_utils import canonical_key
    return device_words(g, canonical_key(g, rng, ks.bits, st_p["moduli"], ks.digits * 2 * ks.mod_count,
                                         1 << ks.n_power), offset)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9])
@pytest.mark.parametrize("L", [1, 3, 5])
def test_bfv_multiply_relinearize_every_output_word(g, bits, n_power, L):
    """all four form combinations, counts 1 and 3, K_b from the bound, K_p = 2, alpha = 2; at n_power <= 5 and count 1
    against Python integers too; a squaring; out over x, then over y"""
    import torch
    _, st_b, st_p, bfv, ks = bfv_plans(g, bits, n_power, L)
    n, t = 1 << n_power, bfv.plain_modulus
    rng = np.random.default_rng(bits + 10 * n_power + L)
    key = bfv_key(g, rng, ks, st_p)
    cases = None
    if n_power <= 5:
        M_all = 2 * L + 6
        all_cases = host_cases(bits, n_power, (60, 59, 58, 57) if bits == 64 else (30, 29, 28, 27), M_all)
        K_b = bfv.b_count
        cases = (all_cases[:L + K_b], all_cases[:L] + all_cases[L + K_b:L + K_b + 2])
        assert [c.q for c in cases[0]] == st_b["moduli"] and [c.q for c in cases[1]] == st_p["moduli"]
    for count in (1, 3):
        any_x, any_y = operands(g, rng, bits, st_b["moduli"], L, count, n)
        res_x, res_y = (reduced(g, v, st_b["moduli"][:L], n, bits) for v in (any_x, any_y))
        keep = [v.clone() for v in (any_x, any_y, res_x, res_y, key)]
        scratch, ks_scratch = bfv_scratch(bfv, count), relin_scratch(ks, count)
        for input_ntt, output_ntt in FORMS:
            x, y = (res_x, res_y) if input_ntt else (any_x, any_y)
            out = filled(bits, 2 * count * L * n)
            bfv.multiply_relinearize(x, y, ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
            torch.cuda.synchronize()
            want = composition_bfv(g, ks, st_b, st_p, t, x, y, key, count, input_ntt, output_ntt)
            assert torch.equal(out, want), (count, input_ntt, output_ntt)
            if cases is not None and count == 1 and input_ntt == output_ntt:
                hx, hy = (from_words(g.to_host(v), (2, count, L, n)) for v in (x, y))
                hkey = from_words(g.to_host(key), (ks.digits, 2, ks.mod_count, n))
                exact = exact_bfv_multiply_relinearize(cases[0], cases[1], L, t, 2, bits, hx, hy, hkey, input_ntt,
                                                       output_ntt)
                assert np.array_equal(from_words(g.to_host(out), exact.shape), exact), (input_ntt, output_ntt)
            if count == 3 and input_ntt == output_ntt:
                xc, yc = x.clone(), y.clone()
                bfv.multiply_relinearize(xc, y, ks, key, xc, count, input_ntt, output_ntt, scratch, ks_scratch)
                bfv.multiply_relinearize(x, yc, ks, key, yc, count, input_ntt, output_ntt, scratch, ks_scratch)
                torch.cuda.synchronize()
                assert torch.equal(xc[:out.numel()], out) and torch.equal(yc[:out.numel()], out), "out over an operand"
                bfv.multiply_relinearize(x, x, ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
                torch.cuda.synchronize()
                assert torch.equal(out, composition_bfv(g, ks, st_b, st_p, t, x, x, key, count, input_ntt,
                                                        output_ntt)), "a squaring"
        assert all(torch.equal(v, k) for v, k in zip((any_x, any_y, res_x, res_y, key), keep)), "an input was modified"


# ------------------------------------------------------------------------------------- launches, memory, refusals
def stage_logs(g, st, mods, n_power, batches, buf):
    """the launch list of each transform alone: name -> (table, direction, moduli, batch)"""
    logs = {}
    for name, (table, kind, mc, batch) in batches.items():
        alone = g.NTTPlan(st[table], mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
        with g.launch_log() as log:
            alone.execute(buf[:batch << n_power], buf[:batch << n_power], batch)
        assert log.kernels
        logs[name] = log.kernels
    return logs


def test_relinearize_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha = 64, 9, 6, 2, 2
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    mods = [c.prm.modulus for c in full.cases[:M]]
    lists = {}
    for count in (1, 3):
        low = 2 * count * L * n
        sbytes = plan.scratch_bytes(count, 2)
        scratch = torch.zeros(sbytes, dtype=torch.uint8, device="cuda:0")
        stages = stage_logs(g, st, mods, n_power, {"inv_q": ("inv", g.INVERSE, L, count * L),
                                                   "fwd_full": ("fwd", g.FORWARD, M, D * count * M),
                                                   "inv_full": ("inv", g.INVERSE, M, 2 * count * M),
                                                   "fwd_q": ("fwd", g.FORWARD, L, 2 * count * L)},
                            scratch.view(torch.int64))
        out = filled(bits, low)
        torch.cuda.synchronize()
        allocs = g.alloc_count()
        for input_ntt, output_ntt in FORMS:
            ct, key = relin3_operands(g, plan, st, np.random.default_rng(5), count, input_ntt)
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            with g.launch_log() as log:
                plan.relinearize(ct[:low], ct[low:], key, out, count, input_ntt, output_ntt, scratch)
            with g.launch_log() as apply_log:
                plan.apply(ct[low:], key, out, count, 2, input_ntt, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == held
            tail = stages["fwd_q"] if output_ntt else []
            if input_ntt:
                want = stages["inv_q"] + ["ks_mod_up"] + stages["fwd_full"] + ["inner_product_seeded"] + \
                    stages["inv_full"] + ["base_convert"] + tail
            else:
                want = ["ks_mod_up"] + stages["fwd_full"] + ["inner_product"] + stages["inv_full"] + ["mod_down_add"] + tail
            assert log.kernels == want, (log.kernels, want)
            assert len(log.kernels) == len(apply_log.kernels)  # not one launch more than the key switch alone
            assert sum(k in ("inner_product", "inner_product_seeded") for k in log.kernels) == 1
            assert sum(k in ("mod_down_add", "base_convert") for k in log.kernels) == 1
            lists[(count, input_ntt, output_ntt)] = [k.split(":")[0] for k in log.kernels]
            del ct, key
        assert g.alloc_count() == allocs
        del out, scratch
    for forms in FORMS:  # no step's launch count grows with count
        assert len(lists[(1,) + forms]) == len(lists[(3,) + forms]), forms

    count = 3
    low, top = 2 * count * L * n, count * L * n
    ct, key = relin3_operands(g, plan, st, np.random.default_rng(6), count, True)
    c01, c2 = ct[:low], ct[low:]
    out = filled(bits, low)
    sbytes = plan.scratch_bytes(count, 2)
    big = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    scratch = big[:sbytes]
    words64 = scratch.view(torch.int64)
    with g.launch_log() as log:
        plan.relinearize(c01, c2, key, out, 0, True, True, scratch)
        plan.mod_down_add(words64, out, out, 0)
    assert log.kernels == []
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    pair = filled(bits, low + 8)  # two buffers 8 words apart: an overlap that is not "exactly"
    call = plan.relinearize
    x = words64[:2 * M * n]
    down = plan.mod_down_add
    refused = [lambda: call(None, c2, key, out, count, True, False, scratch),
               lambda: call(c01, None, key, out, count, True, False, scratch),
               lambda: call(c01, c2, None, out, count, True, False, scratch),
               lambda: call(c01, c2, key, None, count, True, False, scratch),
               lambda: call(c01, c2, key, out, count, True, False, None),
               lambda: call(c01, c2, key, out, -1, True, False, scratch),
               lambda: call(c01, c2, key, out, 1 << 24, True, False, scratch),           # beyond every buffer and limit
               lambda: call(c01, c2, key, out, count, True, False, relin_scratch(plan, count, short=1)),
               lambda: call(c01, c2, key, out, count, True, False, big[8:]),             # not 256-byte aligned
               lambda: call(c01[1:], c2, key, out, count, True, False, scratch),         # too small
               lambda: call(c01, c2[1:], key, out, count, True, False, scratch),
               lambda: call(c01, c2, key[1:], out, count, True, False, scratch),
               lambda: call(c01, c2, key, out[1:], count, True, False, scratch),
               lambda: call(c01.to(torch.int32), c2, key, out, count, True, False, scratch),
               # out over c01 but not exactly; out over c2, over the key; c01 over c2; the scratch over each of them
               lambda: call(pair[:low], c2, key, pair[8:], count, True, False, scratch),
               lambda: call(pair[:low], c2, key, pair[8:], count, False, False, scratch),
               lambda: call(c01, ct[low - 8:low - 8 + top], key, out, count, True, False, scratch),
               lambda: call(c01, out[:top], key, out, count, True, False, scratch),
               lambda: call(c01, c2, key, key[:low], count, True, False, scratch),
               lambda: call(words64[:low], c2, key, out, count, True, False, scratch),
               lambda: call(c01, words64[-top:], key, out, count, True, False, scratch),
               lambda: call(c01, c2, words64[:key.numel()], out, count, True, False, scratch),
               lambda: call(c01, c2, key, words64[-low:], count, True, False, scratch),
               lambda: bare.relinearize(c01, c2, key, out, count, True, False, scratch),  # no transforms
               # mod_down_add: mod_down's refusals, a null addend, an addend over x, over out but not exactly
               lambda: down(None, out[:2 * L * n], out[:2 * L * n], 2),
               lambda: down(x, None, out[:2 * L * n], 2),
               lambda: down(x, out[:2 * L * n], None, 2),
               lambda: down(x, out[:2 * L * n], out[:2 * L * n], -1),
               lambda: down(x, out[:2 * L * n], x[:2 * L * n], 2),                       # out over x
               lambda: down(x, x[8:8 + 2 * L * n], out[:2 * L * n], 2),                  # the addend over x
               lambda: down(x, pair[:2 * L * n], pair[8:8 + 2 * L * n], 2),              # over out, not exactly
               lambda: down(x[1:], out[:2 * L * n], out[:2 * L * n], 2),                 # too small
               lambda: down(x, out[:2 * L * n - 1], out[:2 * L * n], 2)]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


def test_bfv_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L = 64, 9, 3
    n = 1 << n_power
    full, st_b, st_p, bfv, ks = bfv_plans(g, bits, n_power, L)
    rng = np.random.default_rng(7)
    key = bfv_key(g, rng, ks, st_p)
    lists = {}
    for count in (1, 3):
        x, y = operands(g, rng, bits, st_b["moduli"], L, count, n, residues=True)
        out3, out = filled(bits, 3 * count * L * n), filled(bits, 2 * count * L * n)
        scratch, ks_scratch = bfv_scratch(bfv, count), relin_scratch(ks, count)
        torch.cuda.synchronize()
        before, allocs = torch.cuda.memory_allocated(), g.alloc_count()
        for input_ntt, output_ntt in FORMS:
            with g.launch_log() as log:
                bfv.multiply_relinearize(x, y, ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
            with g.launch_log() as parts:
                bfv.multiply(x, y, out3, count, input_ntt, False, scratch)
                ks.apply(out3[2 * count * L * n:], key, out, count, 2, False, output_ntt, ks_scratch)
            torch.cuda.synchronize()
            # multiply(output_ntt = false) plus apply, and the second bfv_scale_round: the low components are never
            # transformed on their own and nothing adds them in a pass of its own
            assert len(log.kernels) == len(parts.kernels) + 1, (log.kernels, parts.kernels)
            assert log.kernels.count("bfv_scale_round") == 2 and log.kernels.count("mod_down_add") == 1
            assert log.kernels.count("inner_product") == 1 and "base_convert" not in log.kernels
            lists[(count, input_ntt, output_ntt)] = len(log.kernels)
        assert torch.cuda.memory_allocated() == before and g.alloc_count() == allocs
    for forms in FORMS:  # no step's launch count grows with count
        assert lists[(1,) + forms] == lists[(3,) + forms], forms

    count = 3
    ct = 2 * count * L * n
    with g.launch_log() as log:
        bfv.multiply_relinearize(x, y, ks, key, out, 0, True, True, scratch, ks_scratch)
    assert log.kernels == []
    # plans that do not match: another q-modulus, another q_count, another ring, another polynomial, no transforms
    assert L + bfv.b_count + 2 <= 2 * L + 5  # the ring's last prime is in none of the bases
    other = full.sub([0, 1, 2 * L + 5] + list(range(L + bfv.b_count, L + bfv.b_count + 2)))
    small = ring(g, bits, n_power - 1, M=2 * L + 6)
    cyclic = ring(g, bits, n_power, M=2 * L + 6, poly=g.X_N_minus)
    p_idx = list(range(L + bfv.b_count, L + bfv.b_count + 2))
    mismatched = [make_plan(g, other, L, 2, n_power, bits),
                  make_plan(g, full.sub(list(range(L - 1)) + p_idx), L - 1, 2, n_power, bits),
                  make_plan(g, small.sub(list(range(L)) + p_idx), L, 2, n_power - 1, bits),
                  make_plan(g, cyclic.sub(list(range(L)) + p_idx), L, 2, n_power, bits),
                  g.KeySwitchPlan(st_p["moduli"][:L], st_p["moduli"][L:], 2, n_power, bits=bits)]
    bare = g.BfvMultiplyPlan(st_b["moduli"][:L], st_b["moduli"][L:], bfv.plain_modulus, n_power, bits=bits)
    for i, wrong in enumerate(mismatched):
        with g.launch_log() as log:
            with pytest.raises(ValueError, match="The key-switching plan does not match!"):
                bfv.multiply_relinearize(x, y, wrong, key, out, count, True, True, scratch, ks_scratch)
        assert log.kernels == [], i
    with pytest.raises(ValueError, match="The key-switching plan does not match!"):
        bare.multiply_relinearize(x, y, ks, key, out, count, True, True, scratch, ks_scratch)
    pair = filled(bits, ct + 8)
    off = torch.zeros(ks.scratch_bytes(count, 2) + 256, dtype=torch.uint8, device="cuda:0")
    s64, k64 = scratch.view(torch.int64), ks_scratch.view(torch.int64)
    call = bfv.multiply_relinearize
    refused = [lambda: call(None, y, ks, key, out, count, True, True, scratch, ks_scratch),
               lambda: call(x, None, ks, key, out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, None, key, out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, None, out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, None, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, out, count, True, True, None, ks_scratch),
               lambda: call(x, y, ks, key, out, count, True, True, scratch, None),
               lambda: call(x, y, ks, key, out, -1, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, out, 1 << 24, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, out, count, True, True, scratch[:-1], ks_scratch),   # too small
               lambda: call(x, y, ks, key, out, count, True, True, scratch, ks_scratch[:-1]),
               lambda: call(x, y, ks, key, out, count, True, True, scratch, off[8:]),           # not 256-byte aligned
               lambda: call(x, y, ks, key[1:], out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, out[1:], count, True, True, scratch, ks_scratch),
               # out over x but not exactly; out over the key; a scratch over an operand, out, the key, the other scratch
               lambda: call(pair[:ct], y, ks, key, pair[8:], count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, key[:ct], count, True, True, scratch, ks_scratch),
               lambda: call(k64[:ct], y, ks, key, out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, k64[:ct], count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, k64[:key.numel()], out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, s64[:key.numel()], out, count, True, True, scratch, ks_scratch),
               lambda: call(x, y, ks, key, out, count, True, True, scratch, scratch[:ks.scratch_bytes(count, 2)])]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and both scratches inside larger sentinel-filled buffers; the inputs unmodified"""
    import torch
    n_power, L, count = 7, 3, 3
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = bfv_plans(g, bits, n_power, L)
    rng = np.random.default_rng(bits)
    key = bfv_key(g, rng, ks, st_p)
    x, y = operands(g, rng, bits, st_b["moduli"], L, count, n, residues=True)
    keep = [v.clone() for v in (x, y, key)]
    want = composition_bfv(g, ks, st_b, st_p, bfv.plain_modulus, x, y, key, count, True, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sb, kb = bfv.scratch_bytes(count), ks.scratch_bytes(count, 2)
    big_s = torch.full((sb + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    big_k = torch.full((kb + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    bfv.multiply_relinearize(x, y, ks, key, big_out[pad:pad + words_out], count, True, True, big_s[256:256 + sb],
                             big_k[256:256 + kb])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    for big, size in ((big_s, sb), (big_k, kb)):
        assert bool((big[:256] == 0xA5).all()) and bool((big[256 + size:] == 0xA5).all())
    assert all(torch.equal(v, k) for v, k in zip((x, y, key), keep)), "an input was modified"
    # relinearize alone, the same way
    ct, rkey = relin3_operands(g, ks, st_p, rng, count, False)
    low = 2 * count * L * n
    keep = [ct.clone(), rkey.clone()]
    want = composition_relinearize(g, ks, st_p, ct[:low], ct[low:], rkey, count, False, True)
    big_out.fill_(0x5A5A5A5A), big_k.fill_(0xA5)
    ks.relinearize(ct[:low], ct[low:], rkey, big_out[pad:pad + low], count, False, True, big_k[256:256 + kb])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + low], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + low:] == 0x5A5A5A5A).all())
    assert bool((big_k[:256] == 0xA5).all()) and bool((big_k[256 + kb:] == 0xA5).all())
    assert torch.equal(ct, keep[0]) and torch.equal(rkey, keep[1]), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """both calls captured once on one stream (a linear capture, no parallel branches) and replayed with new data: the
    same words as the eager calls"""
    import torch
    n_power, L, count = 9, 3, 2
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = bfv_plans(g, bits, n_power, L)
    low = 2 * count * L * n
    key = bfv_key(g, np.random.default_rng(0), ks, st_p)
    x, y = operands(g, np.random.default_rng(0), bits, st_b["moduli"], L, count, n, residues=True)
    ct, _ = relin3_operands(g, ks, st_p, np.random.default_rng(0), count, True)
    out, out2 = filled(bits, low), filled(bits, low)
    scratch, ks_scratch, ks_scratch2 = bfv_scratch(bfv, count), relin_scratch(ks, count), relin_scratch(ks, count)

    def both(s):
        bfv.multiply_relinearize(x, y, ks, key, out, count, True, True, scratch, ks_scratch, stream=s)
        ks.relinearize(ct[:low], ct[low:], key, out2, count, True, True, ks_scratch2, stream=s)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        both(s)
    s.synchronize()
    allocs = g.alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        both(s)
    for seed in (1, 2):
        nx, ny = operands(g, np.random.default_rng(seed), bits, st_b["moduli"], L, count, n, residues=True)
        nct, _ = relin3_operands(g, ks, st_p, np.random.default_rng(seed), count, True)
        x.copy_(nx), y.copy_(ny), ct.copy_(nct), key.copy_(bfv_key(g, np.random.default_rng(seed), ks, st_p))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager, eager2 = filled(bits, low), filled(bits, low)
        spare = relin_scratch(ks, count)
        bfv.multiply_relinearize(x, y, ks, key, eager, count, True, True, bfv_scratch(bfv, count), spare)
        ks.relinearize(ct[:low], ct[low:], key, eager2, count, True, True, spare)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out2, eager2), seed
        assert torch.equal(eager, composition_bfv(g, ks, st_b, st_p, bfv.plain_modulus, x, y, key, count, True, True))
        assert torch.equal(eager2, composition_relinearize(g, ks, st_p, ct[:low], ct[low:], key, count, True, True))
    assert g.alloc_count() == allocs


def test_it_really_multiplies(g):
    """n_power 5, 64-bit words, L = 2, t = 257: two fresh BFV encryptions c0 + c1 s = Delta m + e (mod Q), Delta =
    floor(Q / t), ternary s with h = |s|_1 and ternary e, multiplied and relinearized in one call under a noiseless key
    s^2 -> s, key[d] = (-a_d s + P g_d s^2, a_d), built as test_gpu_relin.test_it_really_multiplies builds it;
    out_0 + out_1 s decrypts to m1 m2 mod (t, X^N + 1).

    The noise against Q / (2 t).  Two parts.
    (a) The BFV tensor term.  multiply returns (d0, d1, d2) with d0 + d1 s + d2 s^2 = Delta m1 m2 + v (mod Q).  Write
    ct_i(s) = Delta m_i + e_i + Q k_i over the integers, |k_i|_inf <= (1 + h) / 2 + 1.  Then t ct_1(s) ct_2(s) / Q =
    Delta m1 m2 + (the cross terms), each a negacyclic product of N terms: m1 e2 + m2 e1 (at most 2 N t), t (k1 e2 + k2 e1)
    (at most 2 N t ((1 + h) / 2 + 1)), t e1 e2 / Q (below 1), the r_t(Q) terms -- Delta t = Q - r_t(Q) with r_t(Q) < t --
    (m1 m2 r / t and (m1 k2 + m2 k1) r, at most N t + 2 N t ((1 + h) / 2 + 1)), and the roundings of scale_round weighted
    by (1, s, s^2): (1 + h + h^2) (1/2 + 1).  With N = 32, h <= 32 and t = 257 all of this is below 2^22.
    (b) The key switch.  The key is noiseless, so the accumulators satisfy A_0 + A_1 s = P d2 s^2 (mod P Q) exactly;
    mod_down_add returns (A_c - [A_c]_P) / P + d_c, each of the TWO ModDowns off from A_c / P by at most 1/2 + 3 K / 2^W
    per coefficient, and (1, s) weighs them by 1 + h: out_0 + out_1 s - (d0 + d1 s + d2 s^2) is at most (1 + h) / 2 + 1.
    The test asserts (b) against the three components multiply returns for the same operands, and that the whole noise
    stays below Q / (2 t) ~ 2^110, which is what a correct decryption means."""
    import torch
    bits, n_power, L, t, count = 64, 5, 2, 257, 1
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = bfv_plans(g, bits, n_power, L, t=t)
    full, qs, ps = st_p["moduli"], st_p["moduli"][:L], st_p["moduli"][L:]
    M = len(full)
    Q, P = math.prod(qs), math.prod(ps)
    rng = np.random.default_rng(8)
    s = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
    h = int(sum(abs(v) for v in s))
    s2 = negacyclic(s, s)
    assert ks.digits == 1  # alpha = 2 = L: one digit, g_0 = 1
    a_0 = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(n)], dtype=object)
    b_0 = -negacyclic(a_0, s) + P * s2
    key = np.zeros((1, 2, M, n), dtype=object)
    for m, q in enumerate(full):
        key[0, 0, m], key[0, 1, m] = b_0 % q, a_0 % q
    d_key = device_words(g, words(g, key, bits))
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)
    g.GPU_NTT_Inplace(d_key, st_p["fwd"], st_p["mods"], cfg_f, 2 * M, M)

    def encrypt(m):
        a = np.array([int.from_bytes(rng.bytes(32), "little") % Q for _ in range(n)], dtype=object)
        e = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
        c0 = ((Q // t) * m + e - negacyclic(a, s)) % Q
        return device_words(g, words(g, np.array([[c % q for q in qs] for c in (c0, a)], dtype=object), bits))

    m1 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    m2 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    x, y = encrypt(m1), encrypt(m2)
    out, three = filled(bits, 2 * L * n), filled(bits, 3 * L * n)
    bfv.multiply_relinearize(x, y, ks, d_key, out, count, False, False, bfv_scratch(bfv, count), relin_scratch(ks, count))
    bfv.multiply(x, y, three, count, False, False, bfv_scratch(bfv, count))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    d = [crt(c, qs) for c in from_words(g.to_host(three), (3, L, n))]
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    switch = [abs(int(v)) for v in centre((value - d[0] - negacyclic(d[1], s) - negacyclic(d[2], s2)) % Q, Q)]
    bound = (1 + h) / 2 + 1
    v = centre(value % Q, Q)
    noise = [abs(int(e)) for e in centre((v - (Q // t) * (negacyclic(m1, m2) % t)) % Q, Q)]
    print("key switch error %d, bound %.1f; noise 2^%.1f of Q / (2 t) = 2^%.1f"
          % (max(switch), bound, math.log2(max(noise) + 1), math.log2(Q / (2 * t))))
    assert max(switch) <= bound, (max(switch), bound)
    assert 2 * t * max(noise) < Q
    assert np.array_equal(((2 * t * v + Q) // (2 * Q)) % t, negacyclic(m1, m2) % t)


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_bfv_relinearize.cpp, compiled here against include/ and libgpuntt.so: two messages encrypted on
    the host, multiplied and relinearized through the C++ class, decrypted with (1, s) on the host; it prints its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_bfv_relinearize")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_bfv_relinearize.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("10",), ("5", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
