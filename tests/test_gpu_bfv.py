"""BfvMultiplyPlan on the MI355X (include/gpuntt/rns/bfv_multiply.cuh): extend, scale_round and multiply.  Every
comparison is torch.equal against a composition of the public calls that existed before (bfv_utils) on the same device
data, or array_equal against the host references and bfv_exact's Python integers."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bfv_exact import exact_multiply
from bfv_utils import (aux_count, bfv_scratch, composition_extend, composition_multiply, composition_scale_round,
                       make_plan, operands, reduced)
from hoisted_exact import NARROW, host_cases
from hoisted_utils import any_words, device_words, filled, ring
from innerprod_utils import from_words
from keyswitch_utils import centre, crt, negacyclic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [1, 2, 5, 9, 12]  # N = 2 at u32: the one-word loader; 2^12: several column tiles per polynomial
COUNTS = (1, 3)
# (L, K forced odd): K from aux_count; L = 5 with an odd K leaves a ragged BC_KB block; L = 17 has K > 16, so both
# conversions cross a 16-term chunk -- at n_power <= 5 only
SHAPES = [(1, False), (3, False), (5, True), (17, False)]
T = {64: (1 << 40) + 15, 32: 65537}


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def plan_for(g, bits, n_power, L, odd=False, t=None, widths=None, poly=None, transforms=True):
    """the ring's first L primes, the smallest auxiliary base behind them (one more prime where `odd` asks for an odd K)"""
    t = T[bits] if t is None else t
    full = ring(g, bits, n_power, M=2 * L + 4, poly=poly, widths=widths)
    K = aux_count(full.moduli, L, t, 1 << n_power)
    K += 1 if odd and K % 2 == 0 else 0
    st = full.sub(list(range(L + K)))
    if transforms:
        return st, make_plan(g, st, L, t, n_power, bits)
    return st, g.BfvMultiplyPlan(st["moduli"][:L], st["moduli"][L:], t, n_power, bits=bits)


def shapes_for(n_power):
    return [s for s in SHAPES if s[0] < 17 or n_power <= 5]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", RINGS)
@pytest.mark.parametrize("offset", [0, 1])
def test_extend_and_scale_round_every_output_word(g, bits, n_power, offset):
    """against the composition on the same device data and against the host references; exactly one kernel each; the
    inputs unmodified; the buffers one word off 16-byte alignment too"""
    import torch
    n, stacks, dt = 1 << n_power, 3, g.np_dtype(bits)
    for L, odd in shapes_for(n_power):
        st, plan = plan_for(g, bits, n_power, L, odd)
        moduli, M, t = st["moduli"], plan.mod_count, plan.plain_modulus
        assert plan.b_count % 2 == 1 or not odd
        rng = np.random.default_rng(bits + n_power + 10 * L + offset)
        hx = any_words(g, rng, bits, stacks * L * n, moduli[:L])
        x = device_words(g, hx, offset)
        keep = x.clone()
        full = filled(bits, stacks * M * n, offset)
        with g.launch_log() as log:
            plan.extend(x, full, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_extend"], log.kernels
        assert torch.equal(full, composition_extend(g, moduli, L, reduced(g, x, moduli[:L], n, bits), stacks, n_power,
                                                    bits)), L
        want = np.zeros(stacks * M * n, dtype=dt)
        g.bfv_reference_extend(moduli[:L], moduli[L:], hx, want, n_power, stacks, bits)
        assert np.array_equal(g.to_host(full), want), L
        assert torch.equal(x, keep), "an input was modified"

        hf = any_words(g, rng, bits, stacks * M * n, moduli)
        f = device_words(g, hf, offset)
        keep = f.clone()
        out = filled(bits, stacks * L * n, offset)
        with g.launch_log() as log:
            plan.scale_round(f, out, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_scale_round"], log.kernels
        assert torch.equal(out, composition_scale_round(g, moduli, L, t, reduced(g, f, moduli, n, bits), stacks,
                                                        n_power, bits)), L
        want = np.zeros(stacks * L * n, dtype=dt)
        g.bfv_reference_scale_round(moduli[:L], moduli[L:], t, hf, want, n_power, stacks, bits)
        assert np.array_equal(g.to_host(out), want), L
        assert torch.equal(f, keep), "an input was modified"


def check_multiply(g, plan, st, rng, counts, exact_cases=None):
    import torch
    bits, n_power, L, t = plan.bits, plan.n_power, plan.q_count, plan.plain_modulus
    n = 1 << n_power
    for count in counts:
        any_x, any_y = operands(g, rng, bits, st["moduli"], L, count, n)
        res_x, res_y = (reduced(g, v, st["moduli"][:L], n, bits) for v in (any_x, any_y))
        keep = [any_x.clone(), any_y.clone(), res_x.clone(), res_y.clone()]
        scratch = bfv_scratch(plan, count)
        for input_ntt, output_ntt in itertools.product((False, True), repeat=2):
            # coefficient form: any words (extend reads them modulo q_m); NTT form: residues, as the transform takes them
            x, y = (res_x, res_y) if input_ntt else (any_x, any_y)
            out = filled(bits, 3 * count * L * n)
            plan.multiply(x, y, out, count, input_ntt, output_ntt, scratch)
            torch.cuda.synchronize()
            want = composition_multiply(g, st, L, t, x, y, count, input_ntt, output_ntt, n_power, bits)
            assert torch.equal(out, want), (count, input_ntt, output_ntt)
            if exact_cases is not None and count == 1 and input_ntt == output_ntt:
                hx, hy = (from_words(g.to_host(v), (2, count, L, n)) for v in (x, y))
                exact, _ = exact_multiply(exact_cases, L, t, bits, hx, hy, input_ntt, output_ntt)
                assert np.array_equal(from_words(g.to_host(out), exact.shape), exact), (input_ntt, output_ntt)
        assert all(torch.equal(v, k) for v, k in zip((any_x, any_y, res_x, res_y), keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,L,odd", [(n_power, L, odd) for n_power in RINGS for L, odd in shapes_for(n_power)])
def test_multiply_every_output_word(g, bits, n_power, L, odd):
    """against the composition for input_ntt x output_ntt -- any-word operands in coefficient form (the composition
    reduces them first), residues in NTT form, where the first step is a transform; at n_power <= 5 against bfv_exact's
    Python integers too"""
    st, plan = plan_for(g, bits, n_power, L, odd)
    cases = None
    if n_power <= 5:
        from hoisted_utils import DEFAULT_WIDTHS
        cases = host_cases(bits, n_power, DEFAULT_WIDTHS[bits], 2 * L + 4)[:plan.mod_count]
        assert [c.q for c in cases] == st["moduli"]
    check_multiply(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COUNTS, cases)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("widths", ["wide", "narrow", "cyclic"])
def test_on_the_widest_primes_a_narrow_ring_and_a_cyclic_one(g, bits, widths):
    n_power, L = 6, 3
    narrow = tuple(NARROW[bits][0] + i for i in range(4))  # too few NTT primes of 20 bits exist for a whole base
    st, plan = plan_for(g, bits, n_power, L, t=257, widths={"wide": "wide", "narrow": narrow, "cyclic": None}[widths],
                        poly=g.X_N_minus if widths == "cyclic" else None)
    check_multiply(g, plan, st, np.random.default_rng(bits), (3,))


@pytest.mark.parametrize("bits", [64, 32])
def test_a_squaring_and_out_over_an_operand(g, bits):
    """y is x: the operand is extended once; out given as x, then as y, each compared with an out-of-place run"""
    import torch
    n_power, L, count = 9, 3, 3
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L)
    t = plan.plain_modulus
    rng = np.random.default_rng(3 + bits)
    x, y = operands(g, rng, bits, st["moduli"], L, count, n, residues=True)
    scratch = bfv_scratch(plan, count)
    words_in, words_out = 2 * count * L * n, 3 * count * L * n
    for input_ntt, output_ntt in ((False, False), (True, True)):
        out = filled(bits, words_out)
        with g.launch_log() as log:
            plan.multiply(x, x, out, count, input_ntt, output_ntt, scratch)
        torch.cuda.synchronize()
        assert log.kernels.count("bfv_extend") == 1
        assert torch.equal(out, composition_multiply(g, st, L, t, x, x, count, input_ntt, output_ntt, n_power, bits))
        plan.multiply(x, y, out, count, input_ntt, output_ntt, scratch)
        xc, yc = filled(bits, words_out), filled(bits, words_out)
        xc[:words_in], yc[:words_in] = x, y
        plan.multiply(xc, y, xc, count, input_ntt, output_ntt, scratch)
        plan.multiply(x, yc, yc, count, input_ntt, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(xc, out) and torch.equal(yc, out), (input_ntt, output_ntt)
        sq = filled(bits, words_out)
        sq[:words_in] = x
        plan.multiply(sq, sq, sq, count, input_ntt, output_ntt, scratch)  # a squaring in place
        plan.multiply(x, x, out, count, input_ntt, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(sq, out), (input_ntt, output_ntt)


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L = 64, 9, 3
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L)
    rng = np.random.default_rng(5)
    logs = {}
    for count in COUNTS:
        x, y = operands(g, rng, bits, st["moduli"], L, count, n, residues=True)
        out = filled(bits, 3 * count * L * n)
        scratch = bfv_scratch(plan, count)
        plan.multiply(x, y, out, count, True, True, scratch)  # (the transforms' first calls may prepare twiddles)
        torch.cuda.synchronize()
        before, allocs = torch.cuda.memory_allocated(), g.alloc_count()
        with g.launch_log() as log:
            plan.multiply(x, y, out, count, True, True, scratch)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before and g.alloc_count() == allocs
        logs[count] = log.kernels
    # [q-base INTT] bfv_extend per operand, the full-base NTT, bfv_tensor, the full-base INTT, bfv_scale_round, [NTT]
    for k in logs.values():
        own = [name for name in k if name.startswith("bfv_")]
        assert own == ["bfv_extend", "bfv_extend", "bfv_tensor", "bfv_scale_round"], k
        i = [k.index("bfv_extend"), len(k) - 1 - k[::-1].index("bfv_extend"), k.index("bfv_tensor"),
             k.index("bfv_scale_round")]
        assert 0 < i[0] and i[0] + 1 < i[1] and i[1] + 1 < i[2] and i[2] + 1 < i[3] < len(k) - 1, k
    assert len(logs[1]) == len(logs[3]), logs  # no step's launch count grows with count
    with g.launch_log() as log:
        plan.multiply(x, y, out, count, False, False, scratch)
    assert log.kernels[0] == "bfv_extend" and log.kernels[1] == "bfv_extend" and log.kernels[-1] == "bfv_scale_round"
    with g.launch_log() as log:
        plan.multiply(x, y, out, 0, True, True, scratch)
        plan.extend(x, out, 0)
        plan.scale_round(x, out, 0)
    assert log.kernels == []
    _, bare = plan_for(g, bits, n_power, L, transforms=False)
    full = filled(bits, 2 * plan.mod_count * n)
    bare.extend(x, full, 2)  # a plan without transforms: extend and scale_round work
    bare.scale_round(full, out, 2)
    torch.cuda.synchronize()
    big = torch.zeros(plan.scratch_bytes(count) + 512, dtype=torch.uint8, device="cuda:0")
    wide = filled(bits, 3 * count * L * n + 2 * n)
    refused = [lambda: plan.multiply(None, y, out, count, True, True, scratch),
               lambda: plan.multiply(x, None, out, count, True, True, scratch),
               lambda: plan.multiply(x, y, None, count, True, True, scratch),
               lambda: plan.multiply(x, y, out, count, True, True, None),                  # a null scratch
               lambda: plan.multiply(x, y, out, count, True, True, big[8:]),               # not 256-byte aligned
               lambda: plan.multiply(x, y, out, count, True, True, big[:64]),              # too small
               lambda: plan.multiply(x, y, out, -1, True, True, scratch),
               lambda: plan.multiply(x, y, x[n:], 1, True, True, scratch),                 # out over x, not exactly x
               lambda: plan.multiply(wide[n:], y, wide, count, True, True, scratch),       # x inside out
               lambda: plan.multiply(x, y, out, count, True, True, x.view(torch.uint8)),   # the scratch over x
               lambda: plan.multiply(x, y, out, count, True, True, out.view(torch.uint8)),  # the scratch over out
               lambda: plan.multiply(x[:2 * count * L * n - 1], y, out, count, True, True, scratch),   # too small
               lambda: bare.multiply(x, y, out, count, True, True, scratch),               # no transforms
               lambda: plan.extend(x, x, 1), lambda: plan.extend(None, full, 1), lambda: plan.extend(x, full, -1),
               lambda: plan.scale_round(full, full, 1), lambda: plan.scale_round(full, None, 1),
               lambda: g.BfvMultiplyPlan(st["moduli"][:L], st["moduli"][L:-1], T[bits], n_power, bits=bits)]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    with pytest.raises(ValueError, match="Auxiliary base too small!"):
        g.BfvMultiplyPlan(st["moduli"][:L], st["moduli"][L:-1], T[bits], n_power, bits=bits)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed(g, bits):
    """multiply captured once on one stream (a linear capture, no parallel branches) and replayed with new data: the
    same words as an eager call; nothing is allocated by the calls"""
    import torch
    n_power, L, count = 9, 3, 2
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L)
    x, y = operands(g, np.random.default_rng(0), bits, st["moduli"], L, count, n, residues=True)
    out = filled(bits, 3 * count * L * n)
    scratch, scratch2 = bfv_scratch(plan, count), bfv_scratch(plan, count)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.multiply(x, y, out, count, True, True, scratch, stream=s)
    s.synchronize()
    allocs = g.alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.multiply(x, y, out, count, True, True, scratch, stream=s)
    nx, ny = operands(g, np.random.default_rng(1), bits, st["moduli"], L, count, n, residues=True)
    x.copy_(nx), y.copy_(ny)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager = filled(bits, out.numel())
    plan.multiply(x, y, eager, count, True, True, scratch2)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(eager, composition_multiply(g, st, L, plan.plain_modulus, x, y, count, True, True, n_power, bits))
    assert g.alloc_count() == allocs


def test_the_gpu_result_decrypts_to_the_product(g):
    """n_power 5: two fresh encryptions multiplied on the GPU, the three components downloaded and decrypted under
    (1, s, s^2) in Python integers"""
    import torch
    bits, n_power, L, t, count = 64, 5, 2, 257, 1
    n = 1 << n_power
    st, plan = plan_for(g, bits, n_power, L, t=t)
    qs = st["moduli"][:L]
    Q = math.prod(qs)
    rng = np.random.default_rng(8)
    s = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)

    def encrypt(m):
        a = np.array([sum(int(rng.integers(0, 1 << 62)) << (62 * i) for i in range(L + 1)) % Q for _ in range(n)],
                     dtype=object)
        e = np.array([int(v) for v in rng.integers(-1, 2, n)], dtype=object)
        c0 = ((Q // t) * m + e - negacyclic(a, s)) % Q
        ct = np.array([[c % q for q in qs] for c in (c0, a)], dtype=object)  # [2][L][N]
        return g.to_device(np.ascontiguousarray(ct.astype(np.uint64).reshape(-1)))

    m1 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    m2 = np.array([int(v) for v in rng.integers(0, t, n)], dtype=object)
    out = filled(bits, 3 * count * L * n)
    plan.multiply(encrypt(m1), encrypt(m2), out, count, False, False, bfv_scratch(plan, count))
    torch.cuda.synchronize()
    d = [crt(c, qs) for c in from_words(g.to_host(out), (3, L, n))]
    v = centre((d[0] + negacyclic(d[1], s) + negacyclic(d[2], negacyclic(s, s))) % Q, Q)
    assert np.array_equal(((2 * t * v + Q) // (2 * Q)) % t, negacyclic(m1, m2) % t)


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_bfv_multiply.cpp, compiled here against include/ and libgpuntt.so: two messages encrypted on the
    host, multiplied through the C++ class, decrypted with (1, s, s^2) on the host; it prints its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_bfv_multiply")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_bfv_multiply.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("10",), ("5", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
