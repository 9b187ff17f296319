"""KeySwitchPlan.multiply_relinearize on the MI355X (include/gpuntt/rns/key_switch.cuh): the product of two ciphertexts
with the top term switched under the relinearization key, in one key switch.  Every comparison is torch.equal against
the definition -- relin_utils.composition_relin, built from the calls that existed before -- on the same device data, or
array_equal against relin_exact's Python integers."""
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
from relin_exact import exact_multiply_relinearize
from relin_utils import composition_relin, relin_operands, relin_scratch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def check_against_the_composition(g, plan, st, rng, counts, km_moduli=None, offset=0):
    import torch
    bits, n, L = plan.bits, 1 << plan.n_power, plan.q_count
    for count in counts:
        x, y, key = relin_operands(g, plan, st, rng, count, km_moduli, offset)
        keep = [t.clone() for t in (x, y, key)]
        scratch = relin_scratch(plan, count)
        for output_ntt in (False, True):
            want = composition_relin(g, plan, st, x, y, key, count, output_ntt)
            out = filled(bits, 2 * count * L * n, offset)
            plan.multiply_relinearize(x, y, key, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (count, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((x, y, key), keep)), "an input was modified"


COUNTS = (1, 3, 5)  # RB = 1; 2 with a ragged tail; 4 with a ragged tail


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 9, 12])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word(g, bits, n_power, L, K, alpha):
    """N = 2 at u32 is below a 16-byte group: the one-word loader; 2^12 has several column tiles per polynomial"""
    M = L + K
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(100 * n_power + L + bits), COUNTS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [6, 12])
@pytest.mark.parametrize("widths", ["wide", "spread"])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_on_the_widest_primes(g, bits, n_power, widths, L, K, alpha):
    """primes of 62/61 and 30/29 bits, and primes spread over the eighth below 2^(W-2): there the fold sum reaches
    [2^(W-1), 3 q), where a signed comparison or a carry lost from the top bit shows"""
    M = L + K
    st = ring(g, bits, n_power, widths=widths).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(n_power + L + bits), COUNTS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 7])
def test_against_exact_integers_on_the_widest_primes(g, bits, n_power):
    """relin_exact: no GPU call and none of the library's arithmetic"""
    import torch
    L, K, alpha, count = 3, 2, 2, 3
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power, widths="wide").sub(list(range(M)))
    cases = host_cases(bits, n_power, WIDE_WIDTHS[bits], M)
    assert [c.q for c in cases] == st["moduli"]
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(bits + n_power), count)
    hx, hy = (from_words(g.to_host(t), (2, count, L, n)) for t in (x, y))
    hkey = from_words(g.to_host(key), (plan.digits, 2, M, n))
    scratch = relin_scratch(plan, count)
    for output_ntt in (False, True):
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize(x, y, key, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        want = exact_multiply_relinearize(cases, L, alpha, bits, hx, hy, hkey, output_ntt)
        assert np.array_equal(from_words(g.to_host(out), want.shape), want), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
def test_twenty_digits(g, bits):
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert plan.digits == 20
    check_against_the_composition(g, plan, st, np.random.default_rng(20 + bits), [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, bits):
    n_power, L, K, alpha = 6, 3, 2, 2
    st = ring(g, bits, n_power, poly=g.X_N_minus).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    check_against_the_composition(g, plan, st, np.random.default_rng(6 + bits), [3])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_key_in_place(g, bits):
    """L = 4 of a key built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_against_the_composition(g, plan, st, np.random.default_rng(bits), [3], km_moduli=full.moduli)


@pytest.mark.parametrize("bits", [64, 32])
def test_squaring_and_out_over_an_operand(g, bits):
    """y is x; out given as x, then as y, each compared with an out-of-place run"""
    import torch
    n_power, L, K, alpha, count = 9, 3, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(3 + bits), count)
    scratch = relin_scratch(plan, count)
    for output_ntt in (False, True):
        out = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize(x, x, key, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(out, composition_relin(g, plan, st, x, x, key, count, output_ntt)), output_ntt
        plan.multiply_relinearize(x, y, key, out, count, output_ntt, scratch)
        xc, yc = x.clone(), y.clone()
        plan.multiply_relinearize(xc, y, key, xc, count, output_ntt, scratch)
        plan.multiply_relinearize(x, yc, key, yc, count, output_ntt, scratch)
        torch.cuda.synchronize()
        assert torch.equal(xc, out) and torch.equal(yc, out), output_ntt
        sq = x.clone()
        plan.multiply_relinearize(sq, sq, key, sq, count, output_ntt, scratch)  # a squaring in place
        torch.cuda.synchronize()
        assert torch.equal(sq, composition_relin(g, plan, st, x, x, key, count, output_ntt)), output_ntt


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """x, y, the key and out one word off 16-byte alignment (the scratch has to be 256-byte aligned)"""
    n_power, L, K, alpha = 7, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, _, key = relin_operands(g, plan, st, np.random.default_rng(1), 1, offset=1)
    assert x.data_ptr() % 16 and key.data_ptr() % 16
    check_against_the_composition(g, plan, st, np.random.default_rng(9 + bits), COUNTS, offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and the scratch inside larger sentinel-filled buffers; the inputs unmodified"""
    import torch
    n_power, L, K, alpha, count = 7, 3, 2, 2, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(bits), count)
    keep = [t.clone() for t in (x, y, key)]
    want = composition_relin(g, plan, st, x, y, key, count, True)
    words_out, pad = 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = plan.scratch_bytes(count, 2)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    plan.multiply_relinearize(x, y, key, big_out[pad:pad + words_out], count, True, big_scratch[256:256 + sbytes])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())
    assert all(torch.equal(t, k) for t, k in zip((x, y, key), keep)), "an input was modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_multiplies(g, bits):
    """A noiseless instance: ternary s with h = |s|_1, two ciphertexts with c0 + c1 s = msg exactly (mod Q), |msg| < 1000,
    and a key that switches s^2 -> s, key[d] = (-a_d s + P g_d s^2, a_d), g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d], built as
    test_gpu_hoisted_sum.test_it_really_computes_a_linear_transform builds its keys.

    Derivation of the bound, that test's.  The digits of d2 = x1 y1 are digits of that polynomial (the g_d sum absorbs
    whatever multiple of Q_d the ModUp added), so the accumulators of the switch satisfy A_0 + A_1 s = P d2 s^2 (mod P Q)
    exactly: the key is noiseless.  The tensor terms join as P d0 and P d1, exact residues, so the stack that reaches
    mod_down holds S_0 + S_1 s = P (d0 + d1 s + d2 s^2) = P msg_x msg_y (mod P Q).  mod_down returns
    (S_c - [S_c]_P) / P per component: each of the TWO ModDowns is off from S_c / P by at most 1/2 + 3 K / 2^W per
    coefficient, and the combination (1, s) weighs them by 1 + h.  The centred error of out_0 + out_1 s - msg_x msg_y is
    therefore at most (1 + h) / 2 + 1."""
    import torch
    n_power, L, K, alpha = 5, 3, 2, 2
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
    for _ in range(2):
        c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
        msg = np.array([int(v) for v in rng.integers(-999, 1000, size=n)], dtype=object)
        c0 = (msg - negacyclic(c1, s)) % Q
        ct = device_words(g, words(g, np.array([[c % q for q in qs] for c in (c0, c1)], dtype=object), bits))
        g.GPU_NTT_Inplace(ct, st["fwd"], st["mods"], cfg_f, 2 * L, L)
        cts.append(ct), msgs.append(msg)
    out = filled(bits, 2 * L * n)
    plan.multiply_relinearize(cts[0], cts[1], d_key, out, 1, False, relin_scratch(plan, 1))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, L, n))
    bound = (1 + h) / 2 + 1
    value = crt(got[0], qs) + negacyclic(crt(got[1], qs), s)
    err = [abs(int(v)) for v in centre((value - negacyclic(msgs[0], msgs[1])) % Q, Q)]
    print("largest error %d, bound %.1f" % (max(err), bound))
    assert max(err) <= bound, (max(err), bound)


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha, count = 64, 9, 6, 2, 2, 3
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(5), count)
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
            plan.multiply_relinearize(x, y, key, out, count, output_ntt, scratch)
        want = ["tensor_top"] + stages["inv_q"] + ["ks_mod_up"] + stages["fwd_full"] + ["inner_product_tensor"] + \
            stages["inv_full"] + ["base_convert"] + (stages["fwd_q"] if output_ntt else [])
        assert log.kernels == want, (log.kernels, want)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    with g.launch_log() as log:
        plan.multiply_relinearize(x, y, key, out, 0, True, scratch)
    assert log.kernels == []
    off = torch.zeros(sbytes + 256, dtype=torch.uint8, device="cuda:0")
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    ct = x.numel()
    pair = filled(bits, ct + 8)  # two ciphertexts 8 words apart: an overlap that is not "exactly"
    call = plan.multiply_relinearize
    refused = [lambda: call(None, y, key, out, count, False, scratch),
               lambda: call(x, None, key, out, count, False, scratch),
               lambda: call(x, y, None, out, count, False, scratch),
               lambda: call(x, y, key, None, count, False, scratch),
               lambda: call(x, y, key, out, count, False, None),
               lambda: call(x, y, key, out, -1, False, scratch),
               lambda: call(x, y, key, out, 1 << 24, False, scratch),                  # beyond every buffer and limit
               lambda: call(x, y, key, out, count, False, relin_scratch(plan, count, short=1)),
               lambda: call(x, y, key, out, count, False, off[8:]),                    # not 256-byte aligned
               lambda: call(x[1:], y, key, out, count, False, scratch),                # too small
               lambda: call(x, y[1:], key, out, count, False, scratch),
               lambda: call(x, y, key[1:], out, count, False, scratch),
               lambda: call(x, y, key, out[1:], count, False, scratch),
               lambda: call(x.to(torch.int32), y, key, out, count, False, scratch),
               # out over x or y, but not exactly; out over the key; out or the scratch over an operand or each other
               lambda: call(pair[:ct], y, key, pair[8:], count, False, scratch),
               lambda: call(x, pair[8:], key, pair[:ct], count, False, scratch),
               lambda: call(x, y, key, key[:ct], count, False, scratch),
               lambda: call(words64[:ct], y, key, out, count, False, scratch),
               lambda: call(x, words64[-ct:], key, out, count, False, scratch),
               lambda: call(x, y, words64[:key.numel()], out, count, False, scratch),
               lambda: call(x, y, key, words64[-ct:], count, False, scratch),
               lambda: bare.multiply_relinearize(x, y, key, out, count, False, scratch)]  # no transforms
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
    n_power, L, K, alpha, count = 9, 3, 2, 2, 2
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    x, y, key = relin_operands(g, plan, st, np.random.default_rng(0), count)
    out = filled(bits, 2 * count * L * n)
    scratch, scratch2 = relin_scratch(plan, count), relin_scratch(plan, count)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.multiply_relinearize(x, y, key, out, count, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.multiply_relinearize(x, y, key, out, count, True, scratch, stream=s)
    for seed in (1, 2):
        nx, ny, nkey = relin_operands(g, plan, st, np.random.default_rng(seed), count)
        x.copy_(nx), y.copy_(ny), key.copy_(nkey)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = filled(bits, 2 * count * L * n)
        plan.multiply_relinearize(x, y, key, eager, count, True, scratch2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed
        assert torch.equal(eager, composition_relin(g, plan, st, x, y, key, count, True)), seed


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_multiply_relin.cpp, compiled here against include/ and libgpuntt.so: two ciphertexts
    multiplied and relinearized, compared with the composition"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_multiply_relin")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_multiply_relin.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
