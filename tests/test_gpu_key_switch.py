"""Hybrid key switching on the MI355X (include/gpuntt/rns/key_switch.cuh).  Every comparison is exact equality of every
output word.  mod_up / mod_down against the header's formulas restated in Python integers (keyswitch_utils) for small
cases and against the library's host references -- pinned to Python integers by tests/test_key_switch_host.py -- for
larger ones, and against the per-digit / per-stack BaseConvPlan composition they replace; the forced output split and
base pointers off 16-byte alignment; apply against the sequence of public calls; a real key switch with a noiseless key;
launch counts, hipGraph replay, caller-owned workspace and scratch, count = 0, and a C++ caller of the public header."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from gpu_utils import MergeCase, distinct_factors_scaled
from innerprod_utils import from_words, moduli, random_words, words
from keyswitch_utils import (SHAPES, centre, crt, negacyclic, ones, partition, planted_input, public_sequence, ref_mod_down,
                             ref_mod_up, tdtype)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYTHON_INTEGER_LIMIT = 1 << 17  # multiply-accumulates above which the expected values come from the host reference


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def bases(bits, L, K):
    ms = moduli(bits, L + K)
    return ms[:L], ms[L:L + K]


def dev(g, x, bits, offset=0):
    """object array -> device tensor; offset: words by which the base pointer is moved off its 16-byte alignment"""
    import torch
    w = words(g, x, bits)
    t = torch.zeros(w.size + offset, dtype=tdtype(bits), device="cuda:0")
    t[offset:] = g.to_device(w)
    return t[offset:]


def expected_mod_up(g, bits, qs, ps, alpha, x, n_power, count, mode):
    """flat words of a [D][count][M][N]"""
    L, M, D = len(qs), len(qs) + len(ps), len(partition(len(qs), alpha))
    if (D * count * M * min(alpha, L)) << n_power <= PYTHON_INTEGER_LIMIT:
        return words(g, ref_mod_up(qs, ps, alpha, x, bits, mode == g.CENTRED), bits)
    a = np.zeros((D * count * M) << n_power, dtype=g.np_dtype(bits))
    return g.keyswitch_reference_mod_up(qs, ps, alpha, words(g, x, bits), a, n_power, count, mode, bits)


def run_mod_up(g, plan, bits, x, count, mode, offset=0):
    """one call on the GPU; returns the flat words of a [D][count][M][N]"""
    import torch
    d_in = dev(g, x, bits, offset)
    size = (plan.digits * count * plan.mod_count) << plan.n_power
    d_a = ones(bits, size, offset)  # an unwritten word shows
    plan.mod_up(d_in, d_a, count, mode)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(d_in), words(g, x, bits)), "in modified"
    return g.to_host(d_a)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_mod_up_every_output_word(g, bits, L, K, alpha, n_power):
    qs, ps = bases(bits, L, K)
    plan = g.KeySwitchPlan(qs, ps, alpha, n_power, bits=bits)
    rng = np.random.default_rng(1000 * L + 10 * K + alpha + n_power + bits)
    for count in (1, 2, 5):
        x = planted_input(rng, bits, qs, (count, L, 1 << n_power))
        for mode in (g.APPROXIMATE, g.CENTRED):
            want = expected_mod_up(g, bits, qs, ps, alpha, x, n_power, count, mode)
            got = run_mod_up(g, plan, bits, x, count, mode)
            assert np.array_equal(got, want), (count, mode)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K,alpha", [(5, 2, 2), (8, 3, 3)])
def test_mod_up_equals_the_per_digit_composition_it_replaces(g, bits, L, K, alpha):
    """per digit: gather the digit's limbs, BaseConvPlan.convert on the GPU, scatter -- in torch"""
    import torch
    n_power, count = 5, 3
    qs, ps = bases(bits, L, K)
    full, M, n = qs + ps, L + K, 1 << n_power
    plan = g.KeySwitchPlan(qs, ps, alpha, n_power, bits=bits)
    rng = np.random.default_rng(L + bits)
    x = planted_input(rng, bits, qs, (count, L, n))
    d_in = dev(g, x, bits).view(count, L, n)
    for mode in (g.APPROXIMATE, g.CENTRED):
        got = from_words(run_mod_up(g, plan, bits, x, count, mode), (plan.digits, count, M, n))
        for d, S in enumerate(partition(L, alpha)):
            S = list(S)
            rest = [m for m in range(M) if m not in S]
            conv = g.BaseConvPlan([qs[i] for i in S], [full[m] for m in rest], bits)
            d_up = ones(bits, count * len(rest) * n)
            conv.convert(d_in[:, S, :].contiguous().view(-1), d_up, n_power, count, mode)
            torch.cuda.synchronize()
            up = from_words(g.to_host(d_up), (count, len(rest), n))
            assert np.array_equal(got[d][:, rest, :], up), (mode, d)
            assert np.array_equal(got[d][:, S, :], x[:, S, :] % np.array([qs[i] for i in S], dtype=object)[None, :, None])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 9])
@pytest.mark.parametrize("L,K", [(1, 1), (5, 2), (3, 3), (40, 24)])
def test_mod_down_every_output_word(g, bits, L, K, n_power):
    """random canonical words, against Python integers (the host reference where that is too slow) and against
    BaseConvPlan.convert_and_divide stack by stack; both sides implement the same band-inclusive formula"""
    import torch
    qs, ps = bases(bits, L, K)
    full, M, n = qs + ps, L + K, 1 << n_power
    plan = g.KeySwitchPlan(qs, ps, 1, n_power, bits=bits)
    down = g.BaseConvPlan(ps, qs, bits)
    rng = np.random.default_rng(100 * L + K + n_power + bits)
    for stacks in (1, 2, 5, 8):
        x = np.stack([random_words(rng, (stacks, n), bits) % q for q in full], axis=1)  # [stacks][M][N]
        d_x = dev(g, x, bits)
        d_out = ones(bits, stacks * L * n)
        plan.mod_down(d_x, d_out, stacks)
        torch.cuda.synchronize()
        got = from_words(g.to_host(d_out), (stacks, L, n))
        assert np.array_equal(from_words(g.to_host(d_x), x.shape), x), "x modified"
        if (stacks * L * K) << n_power <= PYTHON_INTEGER_LIMIT:
            want = ref_mod_down(qs, ps, x, bits)
        else:
            out = np.zeros(stacks * L * n, dtype=g.np_dtype(bits))
            g.keyswitch_reference_mod_down(qs, ps, words(g, x, bits), out, n_power, stacks, bits)
            want = from_words(out, (stacks, L, n))
        assert np.array_equal(got, want), stacks
        xv = d_x.view(stacks, M, n)
        d_each = ones(bits, stacks * L * n).view(stacks, L * n)
        for s in range(stacks):
            down.convert_and_divide(xv[s, L:].contiguous().view(-1), xv[s, :L].contiguous().view(-1), d_each[s],
                                    n_power, 1, g.CENTRED)
        torch.cuda.synchronize()
        assert np.array_equal(from_words(g.to_host(d_each), (stacks, L, n)), got), stacks


@pytest.mark.parametrize("bits", [64, 32])
def test_forced_output_split_changes_no_word(g, bits):
    L, K, alpha, n_power, count = 8, 3, 3, 5, 2
    qs, ps = bases(bits, L, K)
    plan = g.KeySwitchPlan(qs, ps, alpha, n_power, bits=bits)
    x = planted_input(np.random.default_rng(bits), bits, qs, (count, L, 1 << n_power))
    try:
        for mode in (g.APPROXIMATE, g.CENTRED):
            want = words(g, ref_mod_up(qs, ps, alpha, x, bits, mode == g.CENTRED), bits)
            for split in (1, 2, 64):  # 64: clipped to the number of (digit, block) pairs
                g.set_test_hook("keyswitch_split", split)
                assert np.array_equal(run_mod_up(g, plan, bits, x, count, mode), want), (mode, split)
    finally:
        g.set_test_hook("keyswitch_split", 0)


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """the kernels move one word per lane and access: any word-aligned pointer gives the same words"""
    import torch
    L, K, alpha, n_power, count = 5, 2, 2, 5, 2
    qs, ps = bases(bits, L, K)
    n = 1 << n_power
    plan = g.KeySwitchPlan(qs, ps, alpha, n_power, bits=bits)
    rng = np.random.default_rng(3 + bits)
    x = planted_input(rng, bits, qs, (count, L, n))
    want = words(g, ref_mod_up(qs, ps, alpha, x, bits, True), bits)
    assert np.array_equal(run_mod_up(g, plan, bits, x, count, g.CENTRED, offset=1), want)
    xs = np.stack([random_words(rng, (count, n), bits) % q for q in qs + ps], axis=1)
    d_x, d_out = dev(g, xs, bits, 1), ones(bits, count * L * n, 1)
    assert d_x.data_ptr() % 16 and d_out.data_ptr() % 16
    plan.mod_down(d_x, d_out, count)
    torch.cuda.synchronize()
    assert np.array_equal(from_words(g.to_host(d_out), (count, L, n)), ref_mod_down(qs, ps, xs, bits))


# ---------------------------------------------------------------------------------------------------- the pipeline
_rings = {}


class Ring:
    """M NTT primes of the given widths (cycled) with their tables for one (bits, n_power), negacyclic: what the
    pipeline tests share"""

    def __init__(self, g, bits, n_power, M, widths):
        self.cases = [MergeCase(g, bits, n_power, g.X_N_plus, f)
                      for f in distinct_factors_scaled([widths[i % len(widths)] for i in range(M)], n_power)]
        n = 1 << n_power
        dt = g.np_dtype(bits)
        fwd, inv = np.zeros(M * n, dtype=dt), np.zeros(M * n, dtype=dt)
        for i, c in enumerate(self.cases):
            fwd[i * n:i * n + c.prm.root_of_unity_size] = c.prm.forward_table_device_order
            inv[i * n:i * n + c.prm.root_of_unity_size] = c.prm.inverse_table_device_order
        self.g, self.bits, self.n_power, self.n, self.M = g, bits, n_power, n, M
        self.moduli = [c.q for c in self.cases]
        self.n_inv = [c.prm.n_inv for c in self.cases]
        self.fwd, self.inv = g.to_device(fwd), g.to_device(inv)

    def sub(self, idx):
        """the stack of the moduli idx (a list of indices): values, device moduli, tables, n^-1 (host and device)"""
        g, n = self.g, self.n
        sel = np.concatenate([np.arange(i * n, (i + 1) * n) for i in idx])
        import torch
        t = torch.from_numpy(sel).to("cuda:0")
        ninv = [self.n_inv[i] for i in idx]
        return dict(moduli=[self.moduli[i] for i in idx],
                    mods=g.modulus_array_to_device([self.cases[i].prm.modulus for i in idx], self.bits),
                    fwd=self.fwd[t].contiguous(), inv=self.inv[t].contiguous(), n_inv=ninv,
                    d_ninv=g.to_device(np.array(ninv, dtype=g.np_dtype(self.bits))))


WIDTHS = {64: (60, 59, 58, 57), 32: (30, 29, 28, 27)}
WIDE_WIDTHS = {64: (62, 61, 62, 60), 32: (30, 29, 30, 28)}  # the top of what Modulus<T> accepts


def ring(g, bits, n_power, M=8, wide=False):
    key = (bits, n_power, M, wide)
    if key not in _rings:
        _rings[key] = Ring(g, bits, n_power, M, (WIDE_WIDTHS if wide else WIDTHS)[bits])
    return _rings[key]


def make_plan(g, st, L, alpha, n_power, bits, **kw):
    return g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, st["fwd"], st["inv"], st["n_inv"],
                           g.X_N_plus, bits=bits, **kw)


def scratch_for(plan, count, C, short=0):
    import torch
    return torch.zeros(plan.scratch_bytes(count, C) - short, dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [3, 9, 12])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_apply_equals_the_sequence_of_public_calls(g, bits, n_power, L, K, alpha, wide=False):
    import torch
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power, wide=wide).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    inner = g.InnerProductPlan(st["moduli"], bits)
    D = plan.digits
    rng = np.random.default_rng(n_power + L + bits)
    dt = g.np_dtype(bits)
    for C, count in itertools.product((1, 2), (1, 5)):
        c_in = g.to_device(np.concatenate([rng.integers(0, st["moduli"][i % L], size=n, dtype=dt)
                                           for i in range(count * L)]))
        key = g.to_device(np.concatenate([rng.integers(0, st["moduli"][i % M], size=n, dtype=dt)
                                          for i in range(D * C * M)]))
        scratch = scratch_for(plan, count, C)
        for input_ntt, output_ntt in itertools.product((False, True), (False, True)):
            want, _ = public_sequence(g, plan, inner, st, c_in, key, count, C, input_ntt, output_ntt)
            keep = c_in.clone()
            out = ones(bits, C * count * L * n)
            plan.apply(c_in, key, out, count, C, input_ntt, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (C, count, input_ntt, output_ntt)
            assert torch.equal(c_in, keep)
            a = ones(bits, D * count * M * n)
            out2 = ones(bits, C * count * L * n)
            plan.decompose(c_in, a, count, input_ntt, scratch)
            plan.switch_digits(a, key, out2, count, C, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out2, want), (C, count, input_ntt, output_ntt)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [3, 9, 12])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_apply_equals_the_sequence_of_public_calls_on_the_widest_primes(g, bits, n_power, L, K, alpha):
    """primes of 62/61 and 30/29 bits: 2 q passes 2^(W-1)"""
    test_apply_equals_the_sequence_of_public_calls(g, bits, n_power, L, K, alpha, wide=True)


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_uses_the_full_level_key_in_place(g, bits):
    """L = 4 of a key built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    import torch
    n_power, alpha, C, count = 9, 2, 2, 2
    n = 1 << n_power
    limbs = [0, 1, 2, 3, 6, 7]
    st = ring(g, bits, n_power).sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    inner = g.InnerProductPlan(st["moduli"], bits)
    full = ring(g, bits, n_power).moduli
    rng = np.random.default_rng(bits)
    dt = g.np_dtype(bits)
    c_in = g.to_device(np.concatenate([rng.integers(0, st["moduli"][i % 4], size=n, dtype=dt) for i in range(count * 4)]))
    key = g.to_device(np.concatenate([rng.integers(0, full[i % 8], size=n, dtype=dt) for i in range(3 * C * 8)]))
    want, _ = public_sequence(g, plan, inner, st, c_in, key, count, C, True, True, 8, limbs)
    out = ones(bits, C * count * 4 * n)
    plan.apply(c_in, key, out, count, C, True, True, scratch_for(plan, count, C))
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_switches_keys(g, bits, wide=False):
    """A noiseless switching key from s to s': key[d] = (-a_d s' + P g_d s, a_d), g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d].
    Then sum_d x'_d g_d = c (mod Q) whatever multiple of Q_d the approximate ModUp adds, the inner product is
    P (c s mod Q) (mod P Q) in the combination out_0 + out_1 s', and each centred ModDown is off by at most
    1/2 + 3 K / 2^W per unit of |(1, s')|_1: the integer error of out_0 + out_1 s' - c s is at most (1 + h) / 2 + 1."""
    import torch
    n_power, L, K, alpha, C = 5, 3, 2, 2, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power, wide=wide).sub(list(range(M)))
    full, qs, ps = st["moduli"], st["moduli"][:L], st["moduli"][L:]
    Q, P = math.prod(qs), math.prod(ps)
    plan = make_plan(g, st, L, alpha, n_power, bits)
    inner = g.InnerProductPlan(full, bits)
    rng = np.random.default_rng(17 + bits)
    s_old = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    s_new = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    h = int(sum(abs(v) for v in s_new))
    parts = partition(L, alpha)
    key = np.zeros((len(parts), C, M, n), dtype=object)
    for d, S in enumerate(parts):
        Qd = math.prod(qs[i] for i in S)
        gd = (Q // Qd) * pow(Q // Qd, -1, Qd)
        a_d = np.array([int.from_bytes(rng.bytes(64), "little") % (P * Q) for _ in range(n)], dtype=object)
        b_d = -negacyclic(a_d, s_new) + P * gd * s_old
        for m, q in enumerate(full):
            key[d, 0, m], key[d, 1, m] = b_d % q, a_d % q
    d_key = dev(g, key, bits)
    cfg_f = g.ntt_rns_configuration(n_power=n_power, reduction_poly=g.X_N_plus)
    g.GPU_NTT_Inplace(d_key, st["fwd"], st["mods"], cfg_f, len(parts) * C * M, M)
    c = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
    c_in = dev(g, np.array([c % q for q in qs], dtype=object), bits)
    want = centre(negacyclic(c, s_old) % Q, Q)

    def error_of(d_out):
        out = from_words(g.to_host(d_out), (C, L, n))
        got = crt(out[0], qs) + negacyclic(crt(out[1], qs), s_new)
        return [abs(int(v)) for v in centre((got - want) % Q, Q)]

    bound = (1 + h) / 2 + 1
    out = ones(bits, C * L * n)
    plan.apply(c_in, d_key, out, 1, C, False, False, scratch_for(plan, 1, C))
    torch.cuda.synchronize()
    assert max(error_of(out)) <= bound
    cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=g.X_N_plus,
                                    mod_inverse=st["d_ninv"])
    for mode in (g.APPROXIMATE, g.CENTRED):
        a = ones(bits, len(parts) * M * n)
        plan.mod_up(c_in, a, 1, mode)
        g.GPU_NTT_Inplace(a, st["fwd"], st["mods"], cfg_f, len(parts) * M, M)
        acc = ones(bits, C * M * n)
        inner.multiply_accumulate(a, d_key, acc, n_power, len(parts), C, 1)
        g.GPU_INTT_Inplace(acc, st["inv"], st["mods"], cfg_i, C * M, M)
        out = ones(bits, C * L * n)
        plan.mod_down(acc, out, C)
        torch.cuda.synchronize()
        assert max(error_of(out)) <= bound, mode


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_switches_keys_on_the_widest_primes(g, bits):
    test_it_really_switches_keys(g, bits, wide=True)


def test_launches_scratch_workspace_and_count_zero(g):
    import torch
    bits, n_power, L, K, alpha, C, count = 64, 9, 6, 2, 2, 2, 3
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    ws = torch.zeros(g.KeySwitchPlan.workspace_bytes(L, K, alpha, n_power, bits), dtype=torch.uint8, device="cuda:0")
    plan = make_plan(g, st, L, alpha, n_power, bits, workspace=ws)
    assert not plan.owns_workspace and make_plan(g, st, L, alpha, n_power, bits).owns_workspace
    with pytest.raises(ValueError):
        make_plan(g, st, L, alpha, n_power, bits, workspace=ws[:-1])
    D = plan.digits
    c_in = torch.zeros(count * L * n, dtype=torch.int64, device="cuda:0")
    key = torch.zeros(D * C * M * n, dtype=torch.int64, device="cuda:0")
    a, acc = ones(bits, D * count * M * n), ones(bits, C * count * M * n)
    out = ones(bits, C * count * L * n)
    scratch = scratch_for(plan, count, C)
    # what the four transforms launch on their own: the same tables, moduli and batch hint in stand-alone NTTPlans
    mods = [c.prm.modulus for c in ring(g, bits, n_power).cases[:M]]
    stages = {}
    for name, table, kind, mc, buf, batch in (("inv_q", st["inv"], g.INVERSE, L, c_in, count * L),
                                              ("fwd_full", st["fwd"], g.FORWARD, M, a, D * count * M),
                                              ("inv_full", st["inv"], g.INVERSE, M, acc, C * count * M),
                                              ("fwd_q", st["fwd"], g.FORWARD, L, out, C * count * L)):
        alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
        with g.launch_log() as log:
            alone.execute(buf, buf, batch)
        stages[name] = log.kernels
        assert log.kernels
    with g.launch_log() as log:
        plan.mod_up(c_in, a, count)
    assert log.kernels == ["ks_mod_up"], log.kernels
    with g.launch_log() as log:
        plan.mod_down(acc, out, C * count)
    assert log.kernels == ["base_convert"], log.kernels
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for input_ntt, output_ntt in itertools.product((False, True), (False, True)):
        with g.launch_log() as log:
            plan.apply(c_in, key, out, count, C, input_ntt, output_ntt, scratch)
        want = (stages["inv_q"] if input_ntt else []) + ["ks_mod_up"] + stages["fwd_full"] + ["inner_product"] + \
            stages["inv_full"] + ["base_convert"] + (stages["fwd_q"] if output_ntt else [])
        assert log.kernels == want, (log.kernels, want)  # the transforms' launches plus three
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(ValueError):  # scratch is never grown: one byte short is refused
        plan.apply(c_in, key, out, count, C, False, False, scratch_for(plan, count, C, short=1))
    with pytest.raises(ValueError):
        plan.switch_digits(a, key, out, count, C, False, scratch_for(plan, count, C, short=1))
    for call in (lambda: plan.mod_up(c_in, a, 0), lambda: plan.mod_down(acc, out, 0),
                 lambda: plan.apply(c_in, key, out, 0, C, True, True, scratch),
                 lambda: plan.decompose(c_in, a, 0, True, scratch),
                 lambda: plan.switch_digits(a, key, out, 0, C, True, scratch)):
        with g.launch_log() as log:
            call()
        assert log.kernels == []
    tail = scratch.view(torch.int64)
    refused = [lambda: plan.mod_up(c_in, c_in, count), lambda: plan.mod_down(acc, acc, C * count),
               lambda: plan.mod_up(c_in[1:], a, count), lambda: plan.mod_up(c_in, a[1:], count),
               lambda: plan.mod_down(acc[1:], out, C * count), lambda: plan.mod_up(c_in, a, count, 2),
               lambda: plan.mod_up(c_in.to(torch.int32), a, count), lambda: plan.mod_down(acc, out, -1),
               lambda: plan.apply(c_in, key, out, count, 5, False, False, scratch),
               lambda: plan.apply(c_in, key[1:], out, count, C, False, False, scratch),
               lambda: g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits).apply(
                   c_in, key, out, count, C, False, False, scratch),
               # operands inside the scratch, or inside each other
               lambda: plan.switch_digits(tail[-a.numel():], key, out, count, C, False, scratch),
               lambda: plan.switch_digits(a, tail[-key.numel():], out, count, C, False, scratch),
               lambda: plan.switch_digits(a, key, tail[-out.numel():], count, C, False, scratch),
               lambda: plan.apply(tail[:c_in.numel()], key, out, count, C, False, False, scratch),
               lambda: plan.apply(c_in, key, tail[-out.numel():], count, C, False, False, scratch),
               lambda: plan.decompose(a[:c_in.numel()], a, count, False, scratch),
               lambda: plan.decompose(a[-c_in.numel():], a, count, True, scratch),
               lambda: plan.decompose(c_in, tail[8:8 + a.numel()], count, True, scratch)]
    for call in refused:
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                call()
        assert log.kernels == []
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_apply_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    import torch
    n_power, L, K, alpha, C, count = 9, 3, 2, 2, 2, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    dt = g.np_dtype(bits)
    c_in = torch.zeros(count * L * n, dtype=tdtype(bits), device="cuda:0")
    key = torch.zeros(D * C * M * n, dtype=tdtype(bits), device="cuda:0")
    out = ones(bits, C * count * L * n)
    scratch = scratch_for(plan, count, C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.apply(c_in, key, out, count, C, True, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.apply(c_in, key, out, count, C, True, True, scratch, stream=s)
    scratch2 = scratch_for(plan, count, C)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        c_in.copy_(g.to_device(np.concatenate([rng.integers(0, st["moduli"][i % L], size=n, dtype=dt)
                                               for i in range(count * L)])))
        key.copy_(g.to_device(np.concatenate([rng.integers(0, st["moduli"][i % M], size=n, dtype=dt)
                                              for i in range(D * C * M)])))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = ones(bits, C * count * L * n)
        plan.apply(c_in, key, eager, count, C, True, True, scratch2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_key_switch.cpp, compiled here against include/ and libgpuntt.so: the key switch of
    example_inner_product.cpp on one KeySwitchPlan, checked against the host references"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_key_switch")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_key_switch.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12", "3"), ("10", "2", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
