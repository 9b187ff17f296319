"""The KeySwitchPlan family (include/gpuntt/rns/key_switch.cuh) on the MI355X at the ring sizes its numbers are quoted
at: N = 2^13 ... 2^16, u64 and u32.  Above 2^12 the plan's four transforms leave the single tile (the 8192- and
16384-coefficient tiles, two sweeps, the four-polynomial tile of the u64 2^16 forward contiguous pass, the u32
32-coefficients-per-lane kernels), the ModUp / ModDown grids stop splitting their outputs, the hoisted kernels take the
chunk of the library's own LDS rule over many chunks, and the workspace regions grow with N.

  1. mod_up / mod_down: every word against the library's host references (pinned to Python integers by
     tests/test_key_switch_host.py) and a fixed column sample against keyswitch_utils' Python integers, which share no
     code with the library.
  2. apply, decompose + switch_digits, rotate_hoisted, rotate_hoisted_sum, multiply_relinearize,
     multiply_relinearize_sum and (at 2^13 and 2^14) linear_transform_bsgs: every output word against the composition of
     public calls that defines each of them.  At
     u64 2^16 the library's counter of four-polynomial-tile launches must move exactly for the eligible batches; at u64
     2^14 a plan built with batch_hint = 1 must give the words of the default plan; the launch log of apply must be that
     of the stand-alone NTTPlans plus three kernels, with two sweeps per transform where the README says so.
  3. every entry point once per word size at 2^16 on the widest primes against exact Python integers: no GPU call and
     none of the library's arithmetic on the expected side.
  4. a caller-owned workspace and scratches between guard bytes, the hoisted chunk sizes, base pointers off 16-byte
     alignment and one captured graph, all at 2^16.

Every comparison is equality of every output word; outputs are filled with -1 before each call and inputs are compared
with their copies afterwards."""
import itertools
import time

import numpy as np
import pytest

from bsgs_utils import bsgs_elements, bsgs_operands, bsgs_scratch, composition_bsgs, with_absent
from hoisted_exact import NARROW, exact_rotate_hoisted, exact_rotate_hoisted_sum, exact_u, finish, host_cases, transform
from hoisted_sum_utils import composition_sum, make_weights, sum_scratch, with_nones
from hoisted_utils import (WIDE_WIDTHS, any_words, canonical_key, composition, device_words, elements_for, filled,
                           make_plan, ring, tdtype)
from innerprod_utils import from_words, moduli, words
from keyswitch_utils import (column_sample, columns_of, guarded, guards_intact, planted_input, public_sequence,
                             ref_mod_down, ref_mod_up, unmodified)
from relin_exact import exact_multiply_relinearize
from relin_sum_exact import exact_multiply_relinearize_sum
from relin_sum_utils import composition_relin_sum, relin_sum_operands
from relin_utils import composition_relin, relin_operands, relin_scratch

pytestmark = pytest.mark.gpu

N_POWERS = (13, 14, 15, 16)
SHAPE, SHAPE_D3 = (3, 2, 2), (6, 2, 2)  # D = 2, M = 5 and D = 3, M = 8
G, T = 3, 3

# (bits, n_power, prime set, (L, K, alpha)): every ring on the default and the widest primes (62/61 and 30/29 bits: the
# 4 q / 8 q kernels, 4096-coefficient tiles), 45-bit primes at u64 2^16 (the 31 q forward family), D = 3 once per word
RING_CASES = [(bits, n_power, kind, SHAPE) for bits in (64, 32) for n_power in N_POWERS for kind in ("default", "wide")]
RING_CASES += [(64, 16, "narrow", SHAPE), (64, 16, "default", SHAPE_D3), (32, 16, "default", SHAPE_D3)]
rings = pytest.mark.parametrize("bits,n_power,kind,shape", RING_CASES,
                                ids=["u%d-2^%d-%s-L%d" % (b, n, k, s[0]) for b, n, k, s in RING_CASES])


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    yield pkg
    pkg.set_test_hook("contig_p4", "1")
    pkg.set_test_hook("keyswitch_hoist_chunk", 0)


def the_ring(g, bits, n_power, kind):
    """eight primes with their tables, cached by hoisted_utils.ring for the whole module"""
    return ring(g, bits, n_power, M=8, widths={"default": None, "wide": "wide", "narrow": NARROW[bits]}[kind])


class Setup:
    """the stack of one case, its plan -- at u64 2^14 a second one built with batch_hint = 1, whose transforms take the
    two-sweep 4096-coefficient tiles where the default hint takes the 16384-coefficient tile -- and its batch sizes"""

    def __init__(self, g, bits, n_power, kind, shape):
        L, K, alpha = shape
        self.g, self.bits, self.n_power, self.n = g, bits, n_power, 1 << n_power
        self.L, self.M, self.alpha = L, L + K, alpha
        self.full = the_ring(g, bits, n_power, kind)
        self.st = self.full.sub(list(range(L + K)))
        self.plan = make_plan(g, self.st, L, alpha, n_power, bits)
        self.plans = [self.plan]
        if (bits, n_power) == (64, 14):
            self.plans.append(make_plan(g, self.st, L, alpha, n_power, bits, batch_hint=1))
        self.D = self.plan.digits
        # u64 2^16 forward: groups of four polynomials per modulus take the four-polynomial tile.  D = 2: count 2 makes
        # D count and C count = 4 (both forward transforms eligible), counts 1 and 3 make neither; D = 3 needs count 4
        self.p4 = bits == 64 and n_power == 16 and kind in ("default", "narrow")
        self.counts = (1, 2, 3) if self.D == 2 else (1, 2, 3, 4)
        self.qs = self.st["moduli"]

    def canonical(self, rng, mods, polys):
        return device_words(self.g, canonical_key(self.g, rng, self.bits, mods, polys, self.n))

    def fwd_full_p4(self, count):
        """the full-base forward transform of D count M polynomials runs whole groups of four per modulus"""
        return (self.D * count) % 4 == 0

    def fwd_q_p4(self, stacks, output_ntt):
        """the closing q-base forward transform of stacks L polynomials does"""
        return bool(output_ntt) and stacks % 4 == 0


def run_checked(s, eligible, call, out, want, what, prefill=True):
    """call(plan) on every plan of the setup, out against want.  On the rings of the four-polynomial tile: the library's
    launch counter of that tile moves exactly when the batch is eligible and the hook contig_p4 is at 1; eligible calls
    run again with the hook at 0, the counter stays and the words are the same"""
    import torch
    g = s.g
    try:
        for i, plan in enumerate(s.plans):
            for hook in (("1", "0") if s.p4 and eligible else ("1",)):
                if s.p4:
                    g.set_test_hook("contig_p4", hook)
                if prefill:
                    out.fill_(-1)
                before = g.contig_p4_launches() if s.p4 else 0
                call(plan)
                torch.cuda.synchronize()
                if s.p4:
                    moved = g.contig_p4_launches() - before
                    assert (moved > 0) == (eligible and hook == "1"), (what, "contig_p4=" + hook, eligible, moved)
                assert torch.equal(out, want), (what, "plan %d" % i, "contig_p4=" + hook)
    finally:
        if s.p4:
            g.set_test_hook("contig_p4", "1")


# ------------------------------------------------------------------------------- 1. mod_up and mod_down at real sizes
MOD_CASES = [(bits, n_power, shape) for bits in (64, 32) for n_power in N_POWERS for shape in ((3, 2, 2), (8, 3, 3))]
MOD_CASES.append((64, 13, (40, 24, 20)))  # the 64-lane form


@pytest.mark.parametrize("bits,n_power,shape", MOD_CASES,
                         ids=["u%d-2^%d-L%d" % (b, n, s[0]) for b, n, s in MOD_CASES])
def test_mod_up_and_mod_down_every_word_and_a_python_integer_column_sample(g, bits, n_power, shape):
    """count 1 at 2^13: 64 (128-lane) column tiles, below the 512 from which the grids stop splitting the outputs;
    count N = 2^17: at least 512 tiles at either lane count, the unsplit grid with many tiles"""
    import torch
    L, K, alpha = shape
    M, n = L + K, 1 << n_power
    ms = moduli(bits, M)
    qs, ps = ms[:L], ms[L:]
    plan = g.KeySwitchPlan(qs, ps, alpha, n_power, bits=bits)
    D, dt = plan.digits, g.np_dtype(bits)
    big = (1 << 17) >> n_power
    counts = (1,) if L == 40 else (1, big) if n_power == 13 else (big,)
    rng = np.random.default_rng(1000 * n_power + 10 * L + bits)
    for count in counts:
        cols = column_sample(count * n, n_power + count)
        x = planted_input(rng, bits, qs, (count, L, n))
        xw = words(g, x, bits)
        x_cols = np.ascontiguousarray(np.moveaxis(x, 1, 0).reshape(L, count * n)[:, cols])[None]  # [1][L][cols]
        d_in = g.to_device(xw)
        for mode in (g.APPROXIMATE, g.CENTRED):
            d_a = filled(bits, D * count * M * n)
            plan.mod_up(d_in, d_a, count, mode)
            torch.cuda.synchronize()
            got = g.to_host(d_a)
            want = g.keyswitch_reference_mod_up(qs, ps, alpha, xw, np.zeros(D * count * M * n, dtype=dt), n_power,
                                                count, mode, bits)
            assert np.array_equal(got, want), ("mod_up", count, mode)
            exact = ref_mod_up(qs, ps, alpha, x_cols, bits, mode == g.CENTRED)[:, 0]  # [D][M][cols]
            assert np.array_equal(columns_of(got, D, count, M, n, cols), exact), ("mod_up columns", count, mode)
        assert np.array_equal(g.to_host(d_in), xw), "in modified"
        # mod_down: canonical words [stacks][M][N]
        y = np.stack([rng.integers(0, q, size=(count, n), dtype=np.uint64).astype(dt) for q in ms], axis=1)
        yw = np.ascontiguousarray(y.reshape(-1))
        d_x, d_out = g.to_device(yw), filled(bits, count * L * n)
        plan.mod_down(d_x, d_out, count)
        torch.cuda.synchronize()
        got = g.to_host(d_out)
        want = g.keyswitch_reference_mod_down(qs, ps, yw, np.zeros(count * L * n, dtype=dt), n_power, count, bits)
        assert np.array_equal(got, want), ("mod_down", count)
        exact = ref_mod_down(qs, ps, columns_of(yw, 1, count, M, n, cols), bits)  # [1][L][cols]
        assert np.array_equal(columns_of(got, 1, count, L, n, cols), exact), ("mod_down columns", count)
        assert np.array_equal(g.to_host(d_x), yw), "x modified"


# ------------------------------------------------- 2. the pipelines, word for word against their public compositions
@rings
def test_apply_and_decompose_switch_digits_equal_the_public_sequence(g, bits, n_power, kind, shape):
    import torch
    s = Setup(g, bits, n_power, kind, shape)
    L, M, D, n, st = s.L, s.M, s.D, s.n, s.st
    inner = g.InnerProductPlan(st["moduli"], bits)
    rng = np.random.default_rng(n_power + L + bits)
    for count, C in itertools.product(s.counts, (1, 2)):
        c_in = s.canonical(rng, s.qs[:L], count * L)
        key = s.canonical(rng, s.qs, D * C * M)
        keep = [c_in.clone(), key.clone()]
        scratch = torch.zeros(s.plan.scratch_bytes(count, C), dtype=torch.uint8, device="cuda:0")
        out, a = filled(bits, C * count * L * n), filled(bits, D * count * M * n)
        for input_ntt, output_ntt in itertools.product((False, True), (False, True)):
            what = (count, C, input_ntt, output_ntt)
            want, want_a = public_sequence(g, s.plan, inner, st, c_in, key, count, C, input_ntt, output_ntt)
            run_checked(s, s.fwd_full_p4(count) or s.fwd_q_p4(C * count, output_ntt),
                        lambda p: p.apply(c_in, key, out, count, C, input_ntt, output_ntt, scratch),
                        out, want, ("apply",) + what)
            run_checked(s, s.fwd_full_p4(count), lambda p: p.decompose(c_in, a, count, input_ntt, scratch),
                        a, want_a, ("decompose",) + what)
            run_checked(s, s.fwd_q_p4(C * count, output_ntt),
                        lambda p: p.switch_digits(a, key, out, count, C, output_ntt, scratch),
                        out, want, ("switch_digits",) + what)
        unmodified([c_in, key], keep)


def hoisted_operands(s, rng, count, elements):
    """a and c0 of arbitrary words (0, 2^W - 1, q - 1 and q planted), one canonical key per element"""
    g, bits, n = s.g, s.bits, s.n
    a = device_words(g, any_words(g, rng, bits, s.D * count * s.M * n, s.qs))
    c0 = device_words(g, any_words(g, rng, bits, count * s.L * n, s.qs[:s.L]))
    keys = [s.canonical(rng, s.qs, s.D * 2 * s.M) for _ in range(elements)]
    return a, c0, keys


@rings
def test_rotate_hoisted_equals_its_composition(g, bits, n_power, kind, shape):
    import torch
    s = Setup(g, bits, n_power, kind, shape)
    rng = np.random.default_rng(2 * n_power + s.L + bits)
    elts = elements_for(g, n_power, G)
    for count in s.counts:
        a, c0, keys = hoisted_operands(s, rng, count, G)
        keep = [t.clone() for t in (a, c0, *keys)]
        scratch = torch.zeros(s.plan.hoisted_scratch_bytes(count, G), dtype=torch.uint8, device="cuda:0")
        out = filled(bits, G * 2 * count * s.L * s.n)
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            c = c0 if with_c0 else None
            want = composition(g, s.plan, s.st, a, c, keys, elts, count, output_ntt)
            run_checked(s, s.fwd_q_p4(G * 2 * count, output_ntt),
                        lambda p: p.rotate_hoisted(a, c, keys, elts, out, count, output_ntt, scratch),
                        out, want, (count, with_c0, output_ntt))
        unmodified([a, c0, *keys], keep)


@rings
def test_rotate_hoisted_sum_equals_its_composition(g, bits, n_power, kind, shape):
    s = Setup(g, bits, n_power, kind, shape)
    rng = np.random.default_rng(3 * n_power + s.L + bits)
    elts = elements_for(g, n_power, G)
    for count in s.counts:
        a, c0, keys = hoisted_operands(s, rng, count, G)
        weights = make_weights(g, s.plan, s.st, rng, G)
        w = with_nones(weights, 1)  # one weight None
        assert sum(x is None for x in w) == 1
        keep = [t.clone() for t in (a, c0, *keys, *weights)]
        scratch = sum_scratch(s.plan, count)
        out = filled(bits, 2 * count * s.L * s.n)
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            c = c0 if with_c0 else None
            want = composition_sum(g, s.plan, s.st, a, c, keys, elts, w, count, output_ntt)
            run_checked(s, s.fwd_q_p4(2 * count, output_ntt),
                        lambda p: p.rotate_hoisted_sum(a, c, keys, elts, w, out, count, output_ntt, scratch),
                        out, want, (count, with_c0, output_ntt))
        unmodified([a, c0, *keys, *weights], keep)


@rings
def test_multiply_relinearize_equals_its_composition(g, bits, n_power, kind, shape):
    """also with out given as x, and with y is x"""
    s = Setup(g, bits, n_power, kind, shape)
    rng = np.random.default_rng(5 * n_power + s.L + bits)
    for count in s.counts:
        x, y, key = relin_operands(g, s.plan, s.st, rng, count)
        keep = [t.clone() for t in (x, y, key)]
        scratch = relin_scratch(s.plan, count)
        out, over = filled(bits, x.numel()), x.clone()
        for output_ntt in (False, True):
            eligible = s.fwd_full_p4(count) or s.fwd_q_p4(2 * count, output_ntt)
            want = composition_relin(g, s.plan, s.st, x, y, key, count, output_ntt)
            run_checked(s, eligible, lambda p: p.multiply_relinearize(x, y, key, out, count, output_ntt, scratch),
                        out, want, (count, output_ntt))

            def over_x(p):
                over.copy_(x)
                p.multiply_relinearize(over, y, key, over, count, output_ntt, scratch)
            run_checked(s, eligible, over_x, over, want, (count, output_ntt, "out is x"), prefill=False)
            square = composition_relin(g, s.plan, s.st, x, x, key, count, output_ntt)
            run_checked(s, eligible, lambda p: p.multiply_relinearize(x, x, key, out, count, output_ntt, scratch),
                        out, square, (count, output_ntt, "y is x"))
        unmodified([x, y, key], keep)


@rings
def test_multiply_relinearize_sum_equals_its_composition(g, bits, n_power, kind, shape):
    s = Setup(g, bits, n_power, kind, shape)
    rng = np.random.default_rng(7 * n_power + s.L + bits)
    for count in s.counts:
        xs, ys, key = relin_sum_operands(g, s.plan, s.st, rng, count, T)
        keep = [t.clone() for t in xs + ys + [key]]
        scratch = relin_scratch(s.plan, count)
        out = filled(bits, xs[0].numel())
        for output_ntt in (False, True):
            want = composition_relin_sum(g, s.plan, s.st, xs, ys, key, count, output_ntt)
            run_checked(s, s.fwd_full_p4(count) or s.fwd_q_p4(2 * count, output_ntt),
                        lambda p: p.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch),
                        out, want, (count, output_ntt))
        unmodified(xs + ys + [key], keep)


BSGS_CASES = [c for c in RING_CASES if c[1] <= 14]


@pytest.mark.parametrize("bits,n_power,kind,shape", BSGS_CASES,
                         ids=["u%d-2^%d-%s-L%d" % (b, n, k, s[0]) for b, n, k, s in BSGS_CASES])
def test_linear_transform_bsgs_equals_its_composition(g, bits, n_power, kind, shape):
    """(n1, n2, count) = (3, 2, 2), one baby step and one giant step without a key, one absent weight per row: step 3 is
    the only place where the plan's transforms, mod_down and mod_up run over the stacks of all keyed giant steps in one
    batch, and at 2^14 the u64 inverse transform takes two sweeps.  The exact-integer runs stay on small rings
    (test_gpu_bsgs_exact.py): the arithmetic does not depend on N, the reference's time does"""
    s = Setup(g, bits, n_power, kind, shape)
    n1, n2, count = 3, 2, 2
    rng = np.random.default_rng(11 * n_power + s.L + bits)
    a, c0, c1, bkeys, gkeys, weights = bsgs_operands(g, s.plan, s.st, rng, count, n1, n2)
    be, ge = bsgs_elements(g, n_power, n1, null_at=1), bsgs_elements(g, n_power, n2, null_at=0)
    bk, gk = [bkeys[0], None, bkeys[2]], [None, gkeys[1]]
    w = with_absent(weights, 1)
    assert all(sum(x is None for x in row) == 1 for row in w)
    flat = [t for row in weights for t in row]
    keep = [t.clone() for t in (a, c0, c1, *bkeys, *gkeys, *flat)]
    scratch = bsgs_scratch(s.plan, count, n1, n2)
    out = filled(bits, 2 * count * s.L * s.n)
    for output_ntt in (False, True):
        want = composition_bsgs(g, s.plan, s.st, a, c0, c1, bk, be, gk, ge, w, count, output_ntt)
        run_checked(s, False, lambda p: p.linear_transform_bsgs(a, c0, c1, bk, be, gk, ge, w, out, count, output_ntt,
                                                                  scratch),
                    out, want, ("linear_transform_bsgs", output_ntt))
    unmodified([a, c0, c1, *bkeys, *gkeys, *flat], keep)


@pytest.mark.parametrize("bits,n_power", [(64, 15), (64, 16), (32, 16)])
def test_apply_launches_the_stand_alone_transforms_plus_three_kernels_two_sweeps_each(g, bits, n_power):
    """the construction of test_gpu_key_switch.test_launches_scratch_workspace_and_count_zero; u64 from 2^15 and u32 at
    2^16 every transform is two sweeps (README, lazy_tile_log): at least two kernels per stage"""
    import torch
    s = Setup(g, bits, n_power, "default", SHAPE)
    L, M, D, n, st, plan = s.L, s.M, s.D, s.n, s.st, s.plan
    count, C = 2, 2
    c_in = torch.zeros(count * L * n, dtype=tdtype(bits), device="cuda:0")
    key = s.canonical(np.random.default_rng(1), s.qs, D * C * M)
    a, acc = filled(bits, D * count * M * n, value=0), filled(bits, C * count * M * n, value=0)
    out = filled(bits, C * count * L * n)
    scratch = torch.zeros(plan.scratch_bytes(count, C), dtype=torch.uint8, device="cuda:0")
    mods = [c.prm.modulus for c in s.full.cases[:M]]
    stages = {}
    for name, table, kind, mc, buf, batch in (("inv_q", st["inv"], g.INVERSE, L, c_in, count * L),
                                              ("fwd_full", st["fwd"], g.FORWARD, M, a, D * count * M),
                                              ("inv_full", st["inv"], g.INVERSE, M, acc, C * count * M),
                                              ("fwd_q", st["fwd"], g.FORWARD, L, out, C * count * L)):
        alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
        with g.launch_log() as log:
            alone.execute(buf, buf, batch)
        torch.cuda.synchronize()
        alone.close()
        stages[name] = log.kernels
        assert len(log.kernels) >= 2, (name, log.kernels)
    c_in.zero_()
    for input_ntt, output_ntt in itertools.product((False, True), (False, True)):
        with g.launch_log() as log:
            plan.apply(c_in, key, out, count, C, input_ntt, output_ntt, scratch)
        want = (stages["inv_q"] if input_ntt else []) + ["ks_mod_up"] + stages["fwd_full"] + ["inner_product"] + \
            stages["inv_full"] + ["base_convert"] + (stages["fwd_q"] if output_ntt else [])
        assert log.kernels == want, (log.kernels, want)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. exact integers at 2^16, widest primes
ENTRY_POINTS = ["apply", "rotate_hoisted", "rotate_hoisted_sum", "multiply_relinearize", "multiply_relinearize_sum"]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_against_exact_integers_at_2_16_on_the_widest_primes(g, entry, bits):
    """the compositions share kernels with what they check; here the expected words come from Python integers and the
    oracle's transforms alone.  count 1, two elements / two terms, operands of arbitrary words with the extremes
    planted.
    apply: oracle INTT (input_ntt), keyswitch_utils.ref_mod_up (centred), oracle NTT, exact_u with the single element 1
    and no c0, hoisted_exact.finish"""
    import torch
    t0 = time.perf_counter()
    n_power, count = 16, 1
    L, K, alpha = SHAPE
    s = Setup(g, bits, n_power, "wide", SHAPE)
    M, D, n, plan, qs = s.M, s.D, s.n, s.plan, s.qs
    cases = host_cases(bits, n_power, WIDE_WIDTHS[bits], M)
    assert [c.q for c in cases] == qs
    rng = np.random.default_rng(16 + bits)
    host = 0.0

    def integers(t, shape):
        return from_words(g.to_host(t), shape)

    def compare(out, make_want, what):
        nonlocal host
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        want = make_want()
        host += time.perf_counter() - h0
        assert np.array_equal(integers(out, want.shape), want), what

    if entry == "apply":
        key = device_words(g, any_words(g, rng, bits, D * 2 * M * n, qs))
        hkey = integers(key, (D, 2, M, n))
        scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0")
        raw = any_words(g, rng, bits, count * L * n, qs[:L])
        qv = np.array(qs[:L], dtype=raw.dtype)[None, :, None]
        residues = np.ascontiguousarray((raw.reshape(count, L, n) % qv).reshape(-1))
        # coefficients: any words (mod_up reads them modulo q); NTT form: residues, all the inverse transform is
        # defined on
        for input_ntt, output_ntt, w in ((False, True, raw), (True, False, residues)):
            c_in, out = device_words(g, w), filled(bits, 2 * count * L * n)
            plan.apply(c_in, key, out, count, 2, input_ntt, output_ntt, scratch)

            def want():
                x = from_words(w, (count, L, n))
                if input_ntt:
                    x = transform(cases[:L], x, True)
                a = transform(cases, ref_mod_up(qs[:L], qs[L:], alpha, x, bits, True), False)
                u = exact_u(g, qs, L, n_power, s.st["poly"], a, None, [hkey], [1])
                return finish(cases, L, u[0], bits, output_ntt)
            compare(out, want, (input_ntt, output_ntt))
            assert np.array_equal(g.to_host(c_in), w), "c_in modified"
    elif entry in ("rotate_hoisted", "rotate_hoisted_sum"):
        elts = elements_for(g, n_power, 2)
        a = device_words(g, any_words(g, rng, bits, D * count * M * n, qs))
        c0 = device_words(g, any_words(g, rng, bits, count * L * n, qs[:L]))
        keys = [device_words(g, any_words(g, rng, bits, D * 2 * M * n, qs)) for _ in elts]
        ha, hc0 = integers(a, (D, count, M, n)), integers(c0, (count, L, n))
        hkeys = [integers(k, (D, 2, M, n)) for k in keys]
        if entry == "rotate_hoisted":
            out = filled(bits, 2 * 2 * count * L * n)
            plan.rotate_hoisted(a, c0, keys, elts, out, count, True,
                                torch.zeros(plan.hoisted_scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0"))
            compare(out, lambda: exact_rotate_hoisted(g, cases, L, bits, ha, hc0, hkeys, elts, True), entry)
        else:
            weight = make_weights(g, plan, s.st, rng, 1)[0]
            hw = [integers(weight, (M, n)), None]
            out = filled(bits, 2 * count * L * n)
            plan.rotate_hoisted_sum(a, c0, keys, elts, [weight, None], out, count, True, sum_scratch(plan, count))
            compare(out, lambda: exact_rotate_hoisted_sum(g, cases, L, bits, ha, hc0, hkeys, elts, hw, True), entry)
    elif entry == "multiply_relinearize":
        x, y, key = relin_operands(g, plan, s.st, rng, count)
        hx, hy, hkey = integers(x, (2, count, L, n)), integers(y, (2, count, L, n)), integers(key, (D, 2, M, n))
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize(x, y, key, out, count, True, relin_scratch(plan, count))
        compare(out, lambda: exact_multiply_relinearize(cases, L, alpha, bits, hx, hy, hkey, True), entry)
    else:
        xs, ys, key = relin_sum_operands(g, plan, s.st, rng, count, 2)
        hx, hy = [integers(t, (2, count, L, n)) for t in xs], [integers(t, (2, count, L, n)) for t in ys]
        hkey = integers(key, (D, 2, M, n))
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize_sum(xs, ys, key, out, count, True, relin_scratch(plan, count))
        compare(out, lambda: exact_multiply_relinearize_sum(cases, L, alpha, bits, hx, hy, hkey, True), entry)
    print("exact integers, %s u%d: %.1f s, of which %.1f s the host reference"
          % (entry, bits, time.perf_counter() - t0, host))


# ------------------------------------------------------------- 4. workspace, scratch, chunks, alignment, graph at 2^16
def five_entry_points(plan, data, outs, scratches):
    """every pipeline call of the family on one plan; outs / scratches: dicts by entry point"""
    count, C = data["count"], data["C"]
    plan.apply(data["c_in"], data["key_c"], outs["apply"], count, C, True, True, scratches["apply"])
    plan.decompose(data["c_in"], outs["decompose"], count, True, scratches["apply"])
    plan.switch_digits(outs["decompose"], data["key_c"], outs["switch_digits"], count, C, True, scratches["apply"])
    plan.rotate_hoisted(data["a"], data["c0"], data["keys"], data["elts"], outs["rotate_hoisted"], count, True,
                        scratches["rotate_hoisted"])
    plan.rotate_hoisted_sum(data["a"], data["c0"], data["keys"], data["elts"], data["w"], outs["rotate_hoisted_sum"],
                            count, True, scratches["rotate_hoisted_sum"])
    plan.multiply_relinearize(data["xs"][0], data["ys"][0], data["key"], outs["multiply_relinearize"], count, True,
                              scratches["relin"])
    plan.multiply_relinearize_sum(data["xs"], data["ys"], data["key"], outs["multiply_relinearize_sum"], count, True,
                                  scratches["relin"])


@pytest.mark.parametrize("bits", [64, 32])
def test_caller_owned_workspace_and_exact_scratches_between_guards(g, bits):
    """the workspace of exactly workspace_bytes() and every scratch of exactly its size carved out of 0xA5: the words of
    a plan that owns its workspace, no guard byte touched, no device memory allocated by any call"""
    import torch
    n_power, count, C = 16, 2, 2
    L, K, alpha = SHAPE_D3
    s = Setup(g, bits, n_power, "default", SHAPE_D3)
    M, D, n = s.M, s.D, s.n
    wbytes = g.KeySwitchPlan.workspace_bytes(L, K, alpha, n_power, bits)
    big_ws, ws = guarded(wbytes)
    assert ws.numel() == wbytes
    plan = make_plan(g, s.st, L, alpha, n_power, bits, workspace=ws)
    assert not plan.owns_workspace and s.plan.owns_workspace
    rng = np.random.default_rng(4 + bits)
    a, c0, keys = hoisted_operands(s, rng, count, G)
    xs, ys, key = relin_sum_operands(g, plan, s.st, rng, count, T)
    data = dict(count=count, C=C, c_in=s.canonical(rng, s.qs[:L], count * L), key_c=s.canonical(rng, s.qs, D * C * M),
                a=a, c0=c0, keys=keys, elts=elements_for(g, n_power, G),
                w=with_nones(make_weights(g, plan, s.st, rng, G), 1),
                xs=xs, ys=ys, key=key)
    sizes = {"apply": C * count * L * n, "decompose": D * count * M * n, "switch_digits": C * count * L * n,
             "rotate_hoisted": G * 2 * count * L * n, "rotate_hoisted_sum": 2 * count * L * n,
             "multiply_relinearize": 2 * count * L * n, "multiply_relinearize_sum": 2 * count * L * n}
    sbytes = {"apply": plan.scratch_bytes(count, C), "rotate_hoisted": plan.hoisted_scratch_bytes(count, G),
              "rotate_hoisted_sum": plan.hoisted_sum_scratch_bytes(count), "relin": relin_scratch(plan, count).numel()}
    want = {k: filled(bits, v) for k, v in sizes.items()}
    five_entry_points(s.plan, data, want,
                      {k: torch.zeros(v, dtype=torch.uint8, device="cuda:0") for k, v in sbytes.items()})
    torch.cuda.synchronize()
    got = {k: filled(bits, v) for k, v in sizes.items()}
    bigs = {k: guarded(v) for k, v in sbytes.items()}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    five_entry_points(plan, data, got, {k: view for k, (_, view) in bigs.items()})
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    for k in sizes:
        assert torch.equal(got[k], want[k]), k
    assert guards_intact(big_ws), "workspace guard"
    for k, (big, _) in bigs.items():
        assert guards_intact(big), k


@pytest.mark.parametrize("bits", [64, 32])
def test_hoisted_chunks_the_rule_64_slots_and_2_13(g, bits):
    """keyswitch_hoist_chunk at 0 (the LDS-budget rule: a chunk that is neither 64 slots nor the ring, many chunks), 6
    and 13: the composition's words each time"""
    import torch
    n_power, count = 16, 2
    s = Setup(g, bits, n_power, "default", SHAPE_D3)
    rng = np.random.default_rng(13 + bits)
    elts = elements_for(g, n_power, G)
    a, c0, keys = hoisted_operands(s, rng, count, G)
    w = with_nones(make_weights(g, s.plan, s.st, rng, G), 1)
    want = composition(g, s.plan, s.st, a, c0, keys, elts, count, True)
    want_sum = composition_sum(g, s.plan, s.st, a, c0, keys, elts, w, count, True)
    scratch = torch.zeros(s.plan.hoisted_scratch_bytes(count, G), dtype=torch.uint8, device="cuda:0")
    try:
        for chunk in (0, 6, 13):
            g.set_test_hook("keyswitch_hoist_chunk", chunk)
            if chunk == 0:
                assert 6 < g.keyswitch_hoist_chunk(bits, s.D, n_power) < 16
                assert 6 < g.keyswitch_hoist_sum_chunk(bits, s.D, n_power) < 16
            out, out_sum = filled(bits, want.numel()), filled(bits, want_sum.numel())
            s.plan.rotate_hoisted(a, c0, keys, elts, out, count, True, scratch)
            s.plan.rotate_hoisted_sum(a, c0, keys, elts, w, out_sum, count, True, sum_scratch(s.plan, count))
            torch.cuda.synchronize()
            assert torch.equal(out, want), chunk
            assert torch.equal(out_sum, want_sum), chunk
    finally:
        g.set_test_hook("keyswitch_hoist_chunk", 0)


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """a, c0 and out of rotate_hoisted, x and out of mod_down one word off 16-byte alignment: the one-word loaders over
    many chunks and tiles"""
    import torch
    n_power, count = 16, 2
    s = Setup(g, bits, n_power, "default", SHAPE_D3)
    L, M, D, n, plan = s.L, s.M, s.D, s.n, s.plan
    rng = np.random.default_rng(1 + bits)
    elts = elements_for(g, n_power, G)
    a = device_words(g, any_words(g, rng, bits, D * count * M * n, s.qs), 1)
    c0 = device_words(g, any_words(g, rng, bits, count * L * n, s.qs[:L]), 1)
    keys = [s.canonical(rng, s.qs, D * 2 * M) for _ in range(G)]
    out = filled(bits, G * 2 * count * L * n, 1)
    assert a.data_ptr() % 16 and c0.data_ptr() % 16 and out.data_ptr() % 16
    scratch = torch.zeros(plan.hoisted_scratch_bytes(count, G), dtype=torch.uint8, device="cuda:0")
    for output_ntt in (False, True):
        want = composition(g, plan, s.st, a, c0, keys, elts, count, output_ntt)
        out.fill_(-1)
        plan.rotate_hoisted(a, c0, keys, elts, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(out, want), output_ntt
    dt = g.np_dtype(bits)
    y = np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.uint64).astype(dt) for q in s.qs],
                                      axis=1).reshape(-1))
    d_x, d_out = device_words(g, y, 1), filled(bits, count * L * n, 1)
    assert d_x.data_ptr() % 16 and d_out.data_ptr() % 16
    plan.mod_down(d_x, d_out, count)
    torch.cuda.synchronize()
    want = g.keyswitch_reference_mod_down(s.qs[:L], s.qs[L:], y, np.zeros(count * L * n, dtype=dt), n_power, count,
                                          bits)
    assert np.array_equal(g.to_host(d_out), want)
    assert np.array_equal(g.to_host(d_x), y), "x modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_apply_and_multiply_relinearize_sum_in_one_graph_replayed_with_new_data(g, bits):
    """one side stream, a linear capture of the two calls (no parallel branches), replayed with two new data sets and
    compared with eager calls on second scratches"""
    import torch
    n_power, count, C = 16, 2, 2
    s = Setup(g, bits, n_power, "default", SHAPE_D3)
    L, M, D, n, plan = s.L, s.M, s.D, s.n, s.plan

    def data(seed):
        rng = np.random.default_rng(seed)
        xs, ys, key = relin_sum_operands(g, plan, s.st, rng, count, T)
        return [s.canonical(rng, s.qs[:L], count * L), s.canonical(rng, s.qs, D * C * M), key] + xs + ys

    live = data(0)
    c_in, key_c, key, xs, ys = live[0], live[1], live[2], live[3:3 + T], live[3 + T:]
    out_a, out_r = filled(bits, C * count * L * n), filled(bits, 2 * count * L * n)
    sa, sr = (torch.zeros(plan.scratch_bytes(count, C), dtype=torch.uint8, device="cuda:0") for _ in range(2))
    sa2, sr2 = torch.zeros_like(sa), torch.zeros_like(sr)

    def both(o_a, o_r, s_a, s_r, stream=None):
        plan.apply(c_in, key_c, o_a, count, C, True, True, s_a, stream=stream)
        plan.multiply_relinearize_sum(xs, ys, key, o_r, count, True, s_r, stream=stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # eager warm-up on the capture stream
        both(out_a, out_r, sa, sr, side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both(out_a, out_r, sa, sr, side)
    for seed in (1, 2):
        for old, new in zip(live, data(seed)):
            old.copy_(new)
        out_a.fill_(-1), out_r.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager_a, eager_r = filled(bits, out_a.numel()), filled(bits, out_r.numel())
        both(eager_a, eager_r, sa2, sr2)
        torch.cuda.synchronize()
        assert torch.equal(out_a, eager_a) and torch.equal(out_r, eager_r), seed
