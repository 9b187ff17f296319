"""BfvMultiplyPlan.multiply_sum and multiply_relinearize_sum (include/gpuntt/rns/bfv_multiply.cuh) on the MI355X.  Every
word-for-word comparison is torch.equal against the definition -- bfv_sum_utils' compositions of extend, the transforms,
InnerProductPlan.multiply_accumulate, scale_round and relinearize on the same device data -- or array_equal against
bfv_sum_exact's Python integers."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bfv_sum_exact import exact_multiply_relinearize_sum, rounding_bound
from bfv_sum_utils import composition_bfv_sum, composition_multiply_sum, sum_scratch
from bfv_utils import bfv_scratch, operands, reduced
from bfv_utils import make_plan as make_bfv_plan
from hoisted_exact import host_cases
from hoisted_utils import canonical_key, device_words, filled, make_plan
from innerprod_utils import from_words, words
from keyswitch_utils import centre, crt, negacyclic
from relin3_utils import bases, composition_relinearize
from relin_utils import relin_scratch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = list(itertools.product((False, True), repeat=2))
T = {64: (1 << 40) + 15, 32: 65537}
# the terms of the word-for-word cases as (x, y) operand indices: a squaring, a vector shared by several terms on either
# side, a pair listed twice
PAIRS = {1: [(0, 1)], 2: [(0, 1), (2, 2)], 5: [(0, 1), (2, 2), (0, 3), (4, 1), (0, 1)]}


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def sum_plans(g, bits, n_power, L, terms, t=None, widths=None):
    """the ring, the {q, b} and {q, p} stacks and the two plans; the auxiliary base is the smallest that holds `terms`"""
    t = T[bits] if t is None else t
    full, st_b, st_p, _ = bases(g, bits, n_power, L, t * terms, widths=widths)
    bfv, ks = make_bfv_plan(g, st_b, L, t, n_power, bits), make_plan(g, st_p, L, 2, n_power, bits)
    B, Q = math.prod(st_b["moduli"][L:]), math.prod(st_b["moduli"][:L])
    assert bfv.max_terms == min(32, B // (2 * t * (1 << n_power) * Q)) >= terms
    return full, st_b, st_p, bfv, ks


def sum_key(g, rng, ks, st_p):
    return device_words(g, canonical_key(g, rng, ks.bits, st_p["moduli"], ks.digits * 2 * ks.mod_count, 1 << ks.n_power))


def tensors(g, rng, bits, st_b, L, count, n, howmany, residues):
    """`howmany` separate operand tensors T[2][count][L][N]"""
    out = []
    while len(out) < howmany:
        out += list(operands(g, rng, bits, st_b["moduli"], L, count, n, residues=residues))
    return out[:howmany]


def forward_q(g, st, x, polys, L, n_power):
    cfg = g.ntt_rns_configuration(n_power=n_power, reduction_poly=st["poly"])
    out = x.clone()
    g.GPU_NTT_Inplace(out, st["fwd"], st["mods"], cfg, polys, L)
    return out


def check_both_calls(g, bfv, ks, st_b, st_p, ops, pairs, key, count, forms=FORMS, exact=None):
    """multiply_sum and multiply_relinearize_sum against the composition, every word; ops[input_ntt] the operand tensors"""
    import torch
    bits, n_power, L, t = bfv.bits, bfv.n_power, bfv.q_count, bfv.plain_modulus
    n = 1 << n_power
    low = 2 * count * L * n
    for input_ntt in sorted({f[0] for f in forms}):
        xs, ys = [ops[input_ntt][a] for a, _ in pairs], [ops[input_ntt][b] for _, b in pairs]
        U = len({v.data_ptr() for v in xs + ys})
        scratch, ks_scratch = sum_scratch(bfv, count, U), relin_scratch(ks, count)
        m = composition_multiply_sum(g, st_b, L, t, xs, ys, count, input_ntt, False, n_power, bits)
        for output_ntt in sorted({f[1] for f in forms if f[0] == input_ntt}):
            out3, out = filled(bits, 3 * count * L * n), filled(bits, low)
            bfv.multiply_sum(xs, ys, out3, count, input_ntt, output_ntt, scratch)
            bfv.multiply_relinearize_sum(xs, ys, ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
            torch.cuda.synchronize()
            want3 = forward_q(g, st_b, m, 3 * count * L, L, n_power) if output_ntt else m
            assert torch.equal(out3, want3), ("multiply_sum", len(pairs), count, input_ntt, output_ntt)
            want = composition_relinearize(g, ks, st_p, m[:low], m[low:], key, count, False, output_ntt)
            assert torch.equal(out, want), ("multiply_relinearize_sum", len(pairs), count, input_ntt, output_ntt)
            if exact is not None and input_ntt == output_ntt:
                hx = [from_words(g.to_host(v), (2, count, L, n)) for v in ops[input_ntt]]  # one object per tensor
                hkey = from_words(g.to_host(key), (ks.digits, 2, ks.mod_count, n))
                ref = exact_multiply_relinearize_sum(exact[0], exact[1], L, t, 2, bits, [hx[a] for a, _ in pairs],
                                                     [hx[b] for _, b in pairs], hkey, input_ntt, output_ntt)
                assert np.array_equal(from_words(g.to_host(out), ref.shape), ref), (input_ntt, output_ntt)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9])
@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("terms", [1, 2, 5])
def test_every_output_word(g, bits, n_power, L, terms):
    """all four form combinations, counts 1 and 3, K_b from the bound for `terms`, K_p = 2, alpha = 2; N = 2 at u32 is
    below a 16-byte group (the one-word loader); at n_power <= 2 and count 1 against Python integers too"""
    import torch
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, terms)
    n = 1 << n_power
    rng = np.random.default_rng(bits + 10 * n_power + L + 100 * terms)
    key = sum_key(g, rng, ks, st_p)
    exact = None
    if n_power <= 2:
        all_cases = host_cases(bits, n_power, (60, 59, 58, 57) if bits == 64 else (30, 29, 28, 27), 2 * L + 6)
        K_b = bfv.b_count
        exact = (all_cases[:L + K_b], all_cases[:L] + all_cases[L + K_b:L + K_b + 2])
        assert [c.q for c in exact[0]] == st_b["moduli"] and [c.q for c in exact[1]] == st_p["moduli"]
    pairs = PAIRS[terms]
    for count in (1, 3):
        anyw = tensors(g, rng, bits, st_b, L, count, n, 5, False)
        ops = {False: anyw, True: [reduced(g, v, st_b["moduli"][:L], n, bits) for v in anyw]}
        keep = [v.clone() for v in ops[False] + ops[True] + [key]]
        check_both_calls(g, bfv, ks, st_b, st_p, ops, pairs, key, count, exact=exact if count == 1 else None)
        assert all(torch.equal(v, k) for v, k in zip(ops[False] + ops[True] + [key], keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_one_term_returns_the_words_of_multiply_and_multiply_relinearize(g, bits):
    import torch
    n_power, L, count = 7, 3, 3
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, 1)
    rng = np.random.default_rng(bits)
    key = sum_key(g, rng, ks, st_p)
    x, y = operands(g, rng, bits, st_b["moduli"], L, count, n, residues=True)
    scratch, old, ks_scratch = sum_scratch(bfv, count, 2), bfv_scratch(bfv, count), relin_scratch(ks, count)
    assert bfv.sum_scratch_bytes(count, 2) == bfv.sum_scratch_bytes(count, 1) == bfv.scratch_bytes(count)
    for (input_ntt, output_ntt), (a, b) in itertools.product(FORMS, ((x, y), (x, x))):
        out3, want3 = filled(bits, 3 * count * L * n), filled(bits, 3 * count * L * n)
        out, want = filled(bits, 2 * count * L * n), filled(bits, 2 * count * L * n)
        bfv.multiply_sum([a], [b], out3, count, input_ntt, output_ntt, scratch)
        bfv.multiply(a, b, want3, count, input_ntt, output_ntt, old)
        bfv.multiply_relinearize_sum([a], [b], ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
        bfv.multiply_relinearize(a, b, ks, key, want, count, input_ntt, output_ntt, old, ks_scratch)
        torch.cuda.synchronize()
        assert torch.equal(out3, want3) and torch.equal(out, want), (input_ntt, output_ntt, a is b)


@pytest.mark.parametrize("bits", [64, 32])
def test_thirty_two_terms_on_the_widest_primes(g, bits):
    """terms = 32 = BFV_MAX_TERMS with 64 distinct operands at n_power 5: d1 is one exact sum of 64 products modulo the
    widest primes of the width; the auxiliary base is sized for 32 terms"""
    n_power, L, count, terms = 5, 2, 1, 32
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, terms, widths="wide")
    assert bfv.max_terms == 32 and max(st_b["moduli"]).bit_length() == (62 if bits == 64 else 30)
    rng = np.random.default_rng(32 + bits)
    key = sum_key(g, rng, ks, st_p)
    res = tensors(g, rng, bits, st_b, L, count, n, 2 * terms, True)
    pairs = [(2 * i, 2 * i + 1) for i in range(terms)]
    check_both_calls(g, bfv, ks, st_b, st_p, {True: res, False: res}, pairs, key, count,
                     forms=[(True, True), (False, False)])
    # and one operand that is the x and the y of all 32 terms
    check_both_calls(g, bfv, ks, st_b, st_p, {True: res}, [(0, 0)] * terms, key, count, forms=[(True, True)])


@pytest.mark.parametrize("bits", [64, 32])
def test_shared_pointers_are_extended_once_and_change_no_word(g, bits):
    """y[t] is x[t]; one vector shared by all terms; the same pair listed twice: the words of the same call given
    separate copies, and bfv_extend once per distinct pointer"""
    import torch
    n_power, L, count = 6, 3, 2
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, 4)
    rng = np.random.default_rng(bits + 1)
    key = sum_key(g, rng, ks, st_p)
    a, b, c, d = tensors(g, rng, bits, st_b, L, count, n, 4, True)
    shapes = {"squarings": ([a, b, c], [a, b, c], 3), "one vector shared by all terms": ([a, a, a], [b, c, d], 4),
              "shared on the other side": ([b, c, d], [a, a, a], 4), "a pair twice": ([a, c, a], [b, d, b], 4),
              "everything at once": ([a, a, b, a], [a, b, a, b], 2)}
    ks_scratch = relin_scratch(ks, count)
    for name, (xs, ys, U) in shapes.items():
        cx, cy = [v.clone() for v in xs], [v.clone() for v in ys]  # 2 * terms distinct pointers
        out, want = filled(bits, 2 * count * L * n), filled(bits, 2 * count * L * n)
        out3, want3 = filled(bits, 3 * count * L * n), filled(bits, 3 * count * L * n)
        with g.launch_log() as log:
            bfv.multiply_relinearize_sum(xs, ys, ks, key, out, count, True, True, sum_scratch(bfv, count, U), ks_scratch)
        with g.launch_log() as apart:
            bfv.multiply_relinearize_sum(cx, cy, ks, key, want, count, True, True,
                                         sum_scratch(bfv, count, 2 * len(xs)), ks_scratch)
        bfv.multiply_sum(xs, ys, out3, count, False, False, sum_scratch(bfv, count, U))
        bfv.multiply_sum(cx, cy, want3, count, False, False, sum_scratch(bfv, count, 2 * len(xs)))
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(out3, want3), name
        assert log.kernels.count("bfv_extend") == U and apart.kernels.count("bfv_extend") == 2 * len(xs), name
        assert log.kernels.count("bfv_tensor_sum") == apart.kernels.count("bfv_tensor_sum") == 1, name


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


def test_launch_lists_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L = 64, 9, 3
    n = 1 << n_power
    full, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, 5)
    M = bfv.mod_count
    mods = [c.prm.modulus for c in full.cases[:L]] + [c.prm.modulus for c in full.cases[L:M]]
    assert [int(m.value) for m in mods] == st_b["moduli"]
    rng = np.random.default_rng(7)
    key = sum_key(g, rng, ks, st_p)
    lists = {}
    for count, terms in itertools.product((1, 3), (2, 5)):
        U = 2 * terms
        ops = tensors(g, rng, bits, st_b, L, count, n, U, True)
        xs, ys = ops[0::2], ops[1::2]
        out3, out = filled(bits, 3 * count * L * n), filled(bits, 2 * count * L * n)
        scratch, ks_scratch = sum_scratch(bfv, count, U), relin_scratch(ks, count)
        stages = stage_logs(g, st_b, mods, n_power, {"inv_q": ("inv", g.INVERSE, L, 2 * count * L),
                                                     "fwd_full": ("fwd", g.FORWARD, M, 2 * U * count * M),
                                                     "inv_full": ("inv", g.INVERSE, M, 3 * count * M),
                                                     "fwd_q": ("fwd", g.FORWARD, L, 3 * count * L)},
                            scratch.view(torch.int64))
        torch.cuda.synchronize()
        before, allocs = torch.cuda.memory_allocated(), g.alloc_count()
        for input_ntt, output_ntt in FORMS:
            with g.launch_log() as log3:
                bfv.multiply_sum(xs, ys, out3, count, input_ntt, output_ntt, scratch)
            with g.launch_log() as log:
                bfv.multiply_relinearize_sum(xs, ys, ks, key, out, count, input_ntt, output_ntt, scratch, ks_scratch)
            with g.launch_log() as relin:
                ks.relinearize(out3, out3[2 * count * L * n:], key, out, count, False, output_ntt, ks_scratch)
            torch.cuda.synchronize()
            per_operand = (stages["inv_q"] if input_ntt else []) + ["bfv_extend"]
            head = per_operand * U + stages["fwd_full"] + ["bfv_tensor_sum"] + stages["inv_full"]
            assert log3.kernels == head + ["bfv_scale_round"] + (stages["fwd_q"] if output_ntt else []), log3.kernels
            assert log.kernels == head + ["bfv_scale_round"] * 2 + relin.kernels, (log.kernels, relin.kernels)
            rest = [k.split(":")[0] for k in log.kernels[len(per_operand) * U:]]
            lists[(count, terms, input_ntt, output_ntt)] = (len(per_operand), rest)
        assert torch.cuda.memory_allocated() == before and g.alloc_count() == allocs
    for count, forms in itertools.product((1, 3), FORMS):  # only the per-operand entries grow with terms
        assert lists[(count, 2) + forms] == lists[(count, 5) + forms], (count, forms)
    for terms, forms in itertools.product((2, 5), FORMS):  # and nothing grows with count
        assert len(lists[(1, terms) + forms][1]) == len(lists[(3, terms) + forms][1]), (terms, forms)

    count, terms = 3, 2
    ct = 2 * count * L * n
    a, b, c, d = tensors(g, rng, bits, st_b, L, count, n, 4, True)
    xs, ys = [a, c], [b, d]
    out = filled(bits, ct)
    out3 = filled(bits, 3 * count * L * n)
    scratch, ks_scratch = sum_scratch(bfv, count, 4), relin_scratch(ks, count)
    with g.launch_log() as log:
        bfv.multiply_relinearize_sum(xs, ys, ks, key, out, 0, True, True, scratch, ks_scratch)
        bfv.multiply_sum(xs, ys, out3, 0, True, True, scratch)
    assert log.kernels == []

    # terms beyond max_terms(): a plan whose auxiliary base holds exactly three terms (t chosen for it)
    _, st3, _, _ = bases(g, bits, n_power, L, 2)
    room = math.prod(st3["moduli"][L:]) // (2 * n * math.prod(st3["moduli"][:L]))
    t3 = room // 3
    assert 2 <= t3 < 1 << bits and room // t3 == 3
    three = make_bfv_plan(g, st3, L, t3, n_power, bits)
    assert three.max_terms == 3
    big = sum_scratch(three, count, 8)
    three.multiply_sum([a, b, c], [b, c, d], out3, count, True, True, big)  # three terms pass
    with g.launch_log() as log:
        with pytest.raises(ValueError, match="Auxiliary base too small for these terms!"):
            three.multiply_sum([a, b, c, d], [b, c, d, a], out3, count, True, True, big)
        with pytest.raises(ValueError, match="Invalid terms!"):
            bfv.multiply_sum([], [], out3, count, True, True, scratch)
        with pytest.raises(ValueError, match="Invalid terms!"):
            bfv.multiply_sum([a] * 33, [b] * 33, out3, count, True, True, scratch)
    assert log.kernels == []

    mismatched = [make_plan(g, full.sub(list(range(L - 1)) + [L + bfv.b_count, L + bfv.b_count + 1]), L - 1, 2, n_power,
                            bits),
                  g.KeySwitchPlan(st_p["moduli"][:L], st_p["moduli"][L:], 2, n_power, bits=bits)]
    for wrong in mismatched:
        with pytest.raises(ValueError, match="The key-switching plan does not match!"):
            bfv.multiply_relinearize_sum(xs, ys, wrong, key, out, count, True, True, scratch, ks_scratch)
    pair = filled(bits, ct + 8)
    off = torch.zeros(bfv.sum_scratch_bytes(count, 4) + 256, dtype=torch.uint8, device="cuda:0")
    s64, k64 = scratch.view(torch.int64), ks_scratch.view(torch.int64)
    call, call3 = bfv.multiply_relinearize_sum, bfv.multiply_sum
    args = (count, True, True)
    refused = [lambda: call([a, None], ys, ks, key, out, *args, scratch, ks_scratch),
               lambda: call(xs, [b, None], ks, key, out, *args, scratch, ks_scratch),
               lambda: call(None, ys, ks, key, out, *args, scratch, ks_scratch),
               lambda: call(xs, ys[:1], ks, key, out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, None, key, out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, None, out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, key, None, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, key, out, *args, None, ks_scratch),
               lambda: call(xs, ys, ks, key, out, *args, scratch, None),
               lambda: call(xs, ys, ks, key, out, -1, True, True, scratch, ks_scratch),
               lambda: call(xs, ys, ks, key, out, 1 << 24, True, True, scratch, ks_scratch),
               # the scratch sized for fewer operands than the call has (4 distinct)
               lambda: call(xs, ys, ks, key, out, *args, sum_scratch(bfv, count, 3), ks_scratch),
               lambda: call3(xs, ys, out3, *args, sum_scratch(bfv, count, 2)),
               lambda: call3(xs, ys, out3, *args, bfv_scratch(bfv, count)),
               lambda: call(xs, ys, ks, key, out, *args, scratch, ks_scratch[:-1]),
               lambda: call(xs, ys, ks, key, out, *args, off[8:], ks_scratch),                  # not 256-byte aligned
               lambda: call3(xs, ys, out3, *args, off[8:]),
               lambda: call(xs, ys, ks, key[1:], out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, key, out[1:], *args, scratch, ks_scratch),
               lambda: call3(xs, ys, out3[1:], *args, scratch),
               lambda: call([a, c[1:]], ys, ks, key, out, *args, scratch, ks_scratch),           # an operand too small
               # out over an operand of the second term but not exactly; out over the key; a scratch over an operand of
               # the second term, over out, over the key, over the other scratch
               lambda: call([a, pair[:ct]], ys, ks, key, pair[8:], *args, scratch, ks_scratch),
               lambda: call3(xs, [b, pair[:ct]], pair[8:], count, True, True, scratch),
               lambda: call(xs, ys, ks, key, key[:ct], *args, scratch, ks_scratch),
               lambda: call(xs, [b, k64[:ct]], ks, key, out, *args, scratch, ks_scratch),
               lambda: call([a, s64[-ct:]], ys, ks, key, out, *args, scratch, ks_scratch),
               lambda: call3([a, s64[-ct:]], ys, out3, *args, scratch),
               lambda: call(xs, ys, ks, key, k64[:ct], *args, scratch, ks_scratch),
               lambda: call3(xs, ys, s64[:3 * count * L * n], *args, scratch),
               lambda: call(xs, ys, ks, k64[:key.numel()], out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, s64[:key.numel()], out, *args, scratch, ks_scratch),
               lambda: call(xs, ys, ks, key, out, *args, scratch, scratch[:ks.scratch_bytes(count, 2)])]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    # operands outside [1, 64] have no scratch size
    for operands_ in (0, 65):
        with pytest.raises(ValueError, match="Invalid operands!"):
            bfv.sum_scratch_bytes(count, operands_)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("terms", [2, 3, 8])
def test_one_rounding_against_separate_calls(g, bits, terms):
    """multiply_sum against `terms` calls of multiply added modulo Q: the centred CRT difference per coefficient is within
    the header's unconditional bound (terms + 1) / 2 + terms + 1, and at terms = 3 it is non-zero somewhere -- this call
    rounds t sum D / Q once.  The comparison is made on the three components: the relinearized words of the two sides are
    NOT close word by word (a top component that differs by one decomposes into other digits, and the key multiplies the
    difference), so for multiply_relinearize_sum the same bound is checked where it means something -- through the
    decryption, in test_it_really_multiplies"""
    import torch
    n_power, L, count = 5, 2, 2
    n = 1 << n_power
    _, st_b, _, bfv, _ = sum_plans(g, bits, n_power, L, terms)
    qs = st_b["moduli"][:L]
    Q = math.prod(qs)
    rng = np.random.default_rng(bits + terms)
    ops = tensors(g, rng, bits, st_b, L, count, n, 2 * terms, False)
    xs, ys = ops[0::2], ops[1::2]
    out3, part = filled(bits, 3 * count * L * n), filled(bits, 3 * count * L * n)
    bfv.multiply_sum(xs, ys, out3, count, False, False, sum_scratch(bfv, count, 2 * terms))
    torch.cuda.synchronize()
    total = np.zeros((3 * count, n), dtype=object)
    old = bfv_scratch(bfv, count)
    for x, y in zip(xs, ys):
        bfv.multiply(x, y, part, count, False, False, old)
        torch.cuda.synchronize()
        total += crt(np.moveaxis(from_words(g.to_host(part), (3 * count, L, n)), 1, 0), qs)
    got = crt(np.moveaxis(from_words(g.to_host(out3), (3 * count, L, n)), 1, 0), qs)
    diff = [abs(int(v)) for v in centre((got - total) % Q, Q).reshape(-1)]
    print("terms %d: largest difference %d, bound %.1f, non-zero at %d of %d coefficients"
          % (terms, max(diff), rounding_bound(terms), sum(v != 0 for v in diff), len(diff)))
    assert max(diff) <= rounding_bound(terms), (max(diff), rounding_bound(terms))
    if terms == 3:
        assert max(diff) > 0, "three separate roundings and one rounding agree at every coefficient"


def test_it_really_multiplies(g):
    """three pairs of fresh BFV encryptions at t = 65537, n_power 5, 64-bit words, L = 2: c0 + c1 s = Delta m + e (mod Q),
    ternary s and e, summed, multiplied and relinearized in ONE call under a noiseless key s^2 -> s built as
    test_gpu_relin3.test_it_really_multiplies builds it; out_0 + out_1 s decrypts to sum_t m_t m'_t mod (t, X^N + 1) in
    Python integers.  The noise is at most three times that test's, far below Q / (2 t) ~ 2^102.  Against the three
    components multiply_sum returns for the same operands the key switch adds at most (1 + h) / 2 + 1, as there"""
    import torch
    bits, n_power, L, t, count, terms = 64, 5, 2, 65537, 1, 3
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, terms, t=t)
    full, qs, ps = st_p["moduli"], st_p["moduli"][:L], st_p["moduli"][L:]
    M = len(full)
    Q, P = math.prod(qs), math.prod(ps)
    rng = np.random.default_rng(8)
    s = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
    h = int(sum(abs(v) for v in s))
    s2 = negacyclic(s, s)
    assert ks.digits == 1
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

    ms = [np.array([int(v) for v in rng.integers(0, t, n)], dtype=object) for _ in range(2 * terms)]
    cts = [encrypt(m) for m in ms]
    xs, ys = cts[0::2], cts[1::2]
    want = sum(negacyclic(a, b) for a, b in zip(ms[0::2], ms[1::2])) % t
    out, three = filled(bits, 2 * L * n), filled(bits, 3 * L * n)
    scratch = sum_scratch(bfv, count, 2 * terms)
    bfv.multiply_relinearize_sum(xs, ys, ks, d_key, out, count, False, False, scratch, relin_scratch(ks, count))
    bfv.multiply_sum(xs, ys, three, count, False, False, scratch)
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    d = [crt(c, qs) for c in from_words(g.to_host(three), (3, L, n))]
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    switch = [abs(int(v)) for v in centre((value - d[0] - negacyclic(d[1], s) - negacyclic(d[2], s2)) % Q, Q)]
    v = centre(value % Q, Q)
    noise = [abs(int(e)) for e in centre((v - (Q // t) * want) % Q, Q)]
    print("key switch error %d, bound %.1f; noise 2^%.1f of Q / (2 t) = 2^%.1f"
          % (max(switch), (1 + h) / 2 + 1, math.log2(max(noise) + 1), math.log2(Q / (2 * t))))
    assert max(switch) <= (1 + h) / 2 + 1
    assert 2 * t * max(noise) < Q
    assert np.array_equal(((2 * t * v + Q) // (2 * Q)) % t, want)


@pytest.mark.parametrize("bits", [64, 32])
def test_out_over_an_operand_and_no_stray_writes(g, bits):
    """out exactly one operand (the x of the first term, the y of the last); out and both scratches inside larger
    sentinel-filled buffers; the inputs unmodified"""
    import torch
    n_power, L, count, terms = 7, 3, 3, 3
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, terms)
    rng = np.random.default_rng(bits)
    key = sum_key(g, rng, ks, st_p)
    ops = tensors(g, rng, bits, st_b, L, count, n, 5, True)
    xs, ys = [ops[0], ops[2], ops[0]], [ops[1], ops[3], ops[4]]
    keep = [v.clone() for v in ops + [key]]
    want = composition_bfv_sum(g, ks, st_b, st_p, bfv.plain_modulus, xs, ys, key, count, True, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sb, kb = bfv.sum_scratch_bytes(count, 5), ks.scratch_bytes(count, 2)
    big_s = torch.full((sb + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    big_k = torch.full((kb + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    bfv.multiply_relinearize_sum(xs, ys, ks, key, big_out[pad:pad + words_out], count, True, True, big_s[256:256 + sb],
                                 big_k[256:256 + kb])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    for big, size in ((big_s, sb), (big_k, kb)):
        assert bool((big[:256] == 0xA5).all()) and bool((big[256 + size:] == 0xA5).all())
    assert all(torch.equal(v, k) for v, k in zip(ops + [key], keep)), "an input was modified"
    # multiply_sum, the same way
    want3 = composition_multiply_sum(g, st_b, L, bfv.plain_modulus, xs, ys, count, True, True, n_power, bits)
    big3 = filled(bits, 3 * count * L * n + 2 * pad, value=0x5A5A5A5A)
    big_s.fill_(0xA5)
    bfv.multiply_sum(xs, ys, big3[pad:-pad], count, True, True, big_s[256:256 + sb])
    torch.cuda.synchronize()
    assert torch.equal(big3[pad:-pad], want3)
    assert bool((big3[:pad] == 0x5A5A5A5A).all()) and bool((big3[-pad:] == 0x5A5A5A5A).all())
    assert bool((big_s[:256] == 0xA5).all()) and bool((big_s[256 + sb:] == 0xA5).all())
    # out exactly an operand: x of the first (and third) term, then y of the last
    scratch, ks_scratch = sum_scratch(bfv, count, 5), relin_scratch(ks, count)
    for which in (0, 4):
        mine = [v.clone() for v in ops]
        xs2, ys2 = [mine[0], mine[2], mine[0]], [mine[1], mine[3], mine[4]]
        bfv.multiply_relinearize_sum(xs2, ys2, ks, key, mine[which], count, True, True, scratch, ks_scratch)
        torch.cuda.synchronize()
        assert torch.equal(mine[which], want), which
        assert all(torch.equal(mine[i], ops[i]) for i in range(5) if i != which), which


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    """both calls captured once on one stream (a linear capture, no parallel branches) and replayed with new data: the
    same words as the eager calls and as the composition"""
    import torch
    n_power, L, count, terms = 9, 3, 2, 3
    n = 1 << n_power
    _, st_b, st_p, bfv, ks = sum_plans(g, bits, n_power, L, terms)
    low = 2 * count * L * n
    key = sum_key(g, np.random.default_rng(0), ks, st_p)
    ops = tensors(g, np.random.default_rng(0), bits, st_b, L, count, n, 4, True)
    xs, ys = [ops[0], ops[2], ops[3]], [ops[1], ops[2], ops[0]]  # U = 4: a squaring and a shared vector
    out, out3 = filled(bits, low), filled(bits, 3 * count * L * n)
    scratch, scratch3, ks_scratch = sum_scratch(bfv, count, 4), sum_scratch(bfv, count, 4), relin_scratch(ks, count)

    def both(s):
        bfv.multiply_relinearize_sum(xs, ys, ks, key, out, count, True, True, scratch, ks_scratch, stream=s)
        bfv.multiply_sum(xs, ys, out3, count, True, False, scratch3, stream=s)
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
        new = tensors(g, np.random.default_rng(seed), bits, st_b, L, count, n, 4, True)
        for v, nv in zip(ops, new):
            v.copy_(nv)
        key.copy_(sum_key(g, np.random.default_rng(seed), ks, st_p))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager, eager3 = filled(bits, low), filled(bits, 3 * count * L * n)
        bfv.multiply_relinearize_sum(xs, ys, ks, key, eager, count, True, True, sum_scratch(bfv, count, 4),
                                     relin_scratch(ks, count))
        bfv.multiply_sum(xs, ys, eager3, count, True, False, sum_scratch(bfv, count, 4))
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out3, eager3), seed
        assert torch.equal(eager, composition_bfv_sum(g, ks, st_b, st_p, bfv.plain_modulus, xs, ys, key, count, True,
                                                      True)), seed
    assert g.alloc_count() == allocs


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_bfv_dot_product.cpp, compiled here against include/ and libgpuntt.so: three pairs of messages
    encrypted on the host, their dot product formed through the C++ class in one call, decrypted with (1, s) on the
    host; it prints the digest of the result of each path -- coefficient form, NTT form, and the two calls of the
    definition -- which have to match, and its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_bfv_dot_product")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_bfv_dot_product.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("10",), ("5", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            digests = [ln.split()[-1] for ln in r.stdout.splitlines() if ln.startswith("digest")]
            assert len(digests) == 3 and len(set(digests)) == 1, r.stdout
