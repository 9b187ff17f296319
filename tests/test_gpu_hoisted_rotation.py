"""KeySwitchPlan.rotate_hoisted on the MI355X (include/gpuntt/rns/key_switch.cuh): G rotations from one decomposition.
Every comparison is torch.equal against the definition -- GPU_Automorphism_NTT, switch_digits and the rotated c0 added to
component 0, composed in hoisted_utils.composition from the calls that existed before -- on the same device data."""
import itertools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hoisted_utils import (any_words, canonical_key, composition, device_words, elements_for, filled, make_plan, ring,
                           tdtype)
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


def hoist_scratch(plan, count, G, short=0):
    import torch
    return torch.zeros(plan.hoisted_scratch_bytes(count, G) - short, dtype=torch.uint8, device="cuda:0")


def operands(g, plan, st, rng, count, G, km_moduli=None, offset=0):
    """a and c0 of arbitrary words, G canonical keys"""
    bits, n = plan.bits, 1 << plan.n_power
    L, M, D = plan.q_count, plan.mod_count, plan.digits
    a = device_words(g, any_words(g, rng, bits, D * count * M * n, st["moduli"]), offset)
    c0 = device_words(g, any_words(g, rng, bits, count * L * n, st["moduli"][:L]), offset)
    km = st["moduli"] if km_moduli is None else km_moduli
    keys = [device_words(g, canonical_key(g, rng, bits, km, D * 2 * len(km), n), offset) for _ in range(G)]
    return a, c0, keys


def check_against_the_composition(g, plan, st, rng, combos, km_moduli=None, offset=0):
    import torch
    bits, n = plan.bits, 1 << plan.n_power
    L = plan.q_count
    for G, count in combos:
        elts = elements_for(g, plan.n_power, G)
        a, c0, keys = operands(g, plan, st, rng, count, G, km_moduli, offset)
        keep = [t.clone() for t in (a, c0, *keys)]
        scratch = hoist_scratch(plan, count, G)
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            want = composition(g, plan, st, a, c0 if with_c0 else None, keys, elts, count, output_ntt)
            out = filled(bits, G * 2 * count * L * n, offset)
            plan.rotate_hoisted(a, c0 if with_c0 else None, keys, elts, out, count, output_ntt, scratch)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (G, count, with_c0, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((a, c0, *keys), keep)), "an input was modified"


COMBOS = [(1, 1), (5, 3), (1, 3), (5, 1)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 2, 5, 6, 7, 9])
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_with_chunks_of_64_slots(g, chunk6, bits, n_power, L, K, alpha, widths=None):
    """sub-chunk rings (one polynomial per workgroup), one chunk exactly, then 2 and 8 chunks: the destination chunk
    differs from the source chunk"""
    M = L + K
    st = ring(g, bits, n_power, widths=widths).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert g.keyswitch_hoist_chunk(bits, plan.digits, n_power) == min(6, n_power)
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
    assert n_power - g.keyswitch_hoist_chunk(bits, plan.digits, n_power) >= 1  # at least 2 chunks per polynomial
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
        a, c0, keys = operands(g, plan, st, np.random.default_rng(1), 1, 1)
        plan.rotate_hoisted(a, c0, keys * 65, [1] * 65, filled(bits, 65 * 2 * L << n_power), 1, False,
                            hoist_scratch(plan, 1, 64))


@pytest.mark.parametrize("bits", [64, 32])
def test_many_digits_force_a_small_chunk(g, bits, widths=None):
    """(L, K, alpha) = (20, 2, 1): D = 20, 21 rows of LDS per chunk slot"""
    n_power, L, K, alpha = 9, 20, 2, 1
    st = ring(g, bits, n_power, M=L + K, widths=widths).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    assert plan.digits == 20 and g.keyswitch_hoist_chunk(bits, 20, n_power) == (7 if bits == 64 else 8)
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
    g.set_test_hook("keyswitch_hoist_chunk", 0)
    check_against_the_composition(g, plan, st, np.random.default_rng(7 + bits), [(5, 1)])


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_keys_in_place(g, bits):
    """L = 4 of keys built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    n_power, alpha = 9, 2
    limbs = [0, 1, 2, 3, 6, 7]
    full = ring(g, bits, n_power)
    st = full.sub(limbs)
    plan = make_plan(g, st, 4, alpha, n_power, bits, key_mod_count=8, key_limbs=limbs)
    check_against_the_composition(g, plan, st, np.random.default_rng(bits), [(5, 3)], km_moduli=full.moduli)


@pytest.mark.parametrize("bits", [64, 32])
def test_base_pointers_one_word_off_alignment(g, bits):
    """a, c0, the keys and out one word off 16-byte alignment (the scratch has to be 256-byte aligned): same words"""
    n_power, L, K, alpha = 7, 3, 2, 2
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, _, _ = operands(g, plan, st, np.random.default_rng(1), 1, 1, offset=1)
    assert a.data_ptr() % 16
    check_against_the_composition(g, plan, st, np.random.default_rng(9 + bits), [(5, 3)], offset=1)


@pytest.mark.parametrize("bits", [64, 32])
def test_no_stray_writes(g, bits):
    """out and the scratch inside larger sentinel-filled buffers"""
    import torch
    n_power, L, K, alpha, G, count = 7, 3, 2, 2, 5, 3
    n = 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    a, c0, keys = operands(g, plan, st, np.random.default_rng(bits), count, G)
    elts = elements_for(g, n_power, G)
    want = composition(g, plan, st, a, c0, keys, elts, count, True)
    words_out, pad = G * 2 * count * L * n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = plan.hoisted_scratch_bytes(count, G)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    plan.rotate_hoisted(a, c0, keys, elts, big_out[pad:pad + words_out], count, True, big_scratch[256:256 + sbytes])
    torch.cuda.synchronize()
    assert torch.equal(big_out[pad:pad + words_out], want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())


@pytest.mark.parametrize("bits", [64, 32])
def test_it_really_rotates(g, bits):
    """A noiseless instance: c0 + c1 s = m (mod Q), and for k = rotation by 1 and conjugation a key that switches
    sigma_k(s) -> s: key_k[d] = (-a_d s + P g_d sigma_k(s), a_d), g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d].  One
    decompose(c1), one rotate_hoisted with both keys.  sigma_k permutes NTT slots, so the rotated digits are digits of
    sigma_k(c1) (sigma_k commutes with the per-coefficient ModUp up to its sign, which the g_d sum absorbs: sum_d x'_d
    g_d = sigma_k(c1) mod Q whatever multiple of Q_d the ModUp added), the inner product is P (sigma_k(c1) sigma_k(s)
    mod Q) (mod P Q) in the combination out_0 + out_1 s, and each of the two centred ModDowns is off by at most
    1/2 + 3 K / 2^W per unit of |(1, s)|_1 -- the bound of test_it_really_switches_keys: the integer error of
    out_0 + out_1 s - sigma_k(c1 s) is at most (1 + h) / 2 + 1, h = |s|_1.  The c0 term is exact (the identity in the
    header: the same word as adding sigma_k(c0) afterwards) and adds nothing, so out_0 + out_1 s - sigma_k(m), centred
    mod Q, stays within (1 + h) / 2 + 1."""
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
    keys = []
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
    c1 = np.array([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)], dtype=object)
    msg = np.array([int(v) for v in rng.integers(-1000, 1000, size=n)], dtype=object)
    c0 = (msg - negacyclic(c1, s)) % Q
    d_c1 = device_words(g, words(g, np.array([c1 % q for q in qs], dtype=object), bits))
    d_c0 = device_words(g, words(g, np.array([c0 % q for q in qs], dtype=object), bits))
    g.GPU_NTT_Inplace(d_c0, st["fwd"], st["mods"], cfg_f, L, L)
    a = filled(bits, plan.digits * M * n)
    plan.decompose(d_c1, a, 1, False, None)
    out = filled(bits, 2 * 2 * L * n)
    plan.rotate_hoisted(a, d_c0, keys, elts, out, 1, False, hoist_scratch(plan, 1, 2))
    torch.cuda.synchronize()
    got = from_words(g.to_host(out), (2, 2, L, n))
    bound = (1 + h) / 2 + 1
    for i, k in enumerate(elts):
        value = crt(got[i, 0], qs) + negacyclic(crt(got[i, 1], qs), s)
        err = [abs(int(v)) for v in centre((value - sigma(msg, k)) % Q, Q)]
        assert max(err) <= bound, (k, max(err), bound)


def test_launches_memory_count_zero_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha, count = 64, 9, 6, 2, 2, 3
    M, n = L + K, 1 << n_power
    full = ring(g, bits, n_power)
    st = full.sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    D = plan.digits
    a, c0, keys = operands(g, plan, st, np.random.default_rng(5), count, 5)
    mods = [c.prm.modulus for c in full.cases[:M]]
    torch.cuda.synchronize()
    for G in (1, 5):
        elts = elements_for(g, n_power, G)
        out = filled(bits, G * 2 * count * L * n)
        scratch = hoist_scratch(plan, count, G)
        stages = {}
        for name, table, kind, mc, buf in (("inv_full", st["inv"], g.INVERSE, M, scratch.view(torch.int64)),
                                           ("fwd_q", st["fwd"], g.FORWARD, L, out)):
            alone = g.NTTPlan(table, mods[:mc], n_power, g.X_N_plus, kind, st["n_inv"][:mc], batch_hint=1024)
            with g.launch_log() as log:
                alone.execute(buf, buf, G * 2 * count * mc)
            stages[name] = log.kernels
            assert log.kernels
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for with_c0, output_ntt in itertools.product((False, True), (False, True)):
            with g.launch_log() as log:
                plan.rotate_hoisted(a, c0 if with_c0 else None, keys[:G], elts, out, count, output_ntt, scratch)
            want = ["inner_product_galois"] + stages["inv_full"] + ["base_convert"] + \
                (stages["fwd_q"] if output_ntt else [])
            assert log.kernels == want, (log.kernels, want)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    G = 5
    with g.launch_log() as log:
        plan.rotate_hoisted(a, c0, keys, elts, out, 0, True, scratch)
    assert log.kernels == []
    tail = scratch.view(torch.int64)
    off = torch.zeros(plan.hoisted_scratch_bytes(count, G) + 256, dtype=torch.uint8, device="cuda:0")
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    call = plan.rotate_hoisted
    refused = [lambda: call(a, c0, [], [], out, count, False, scratch),                       # G = 0
               lambda: call(a, c0, keys * 13, elts * 13, out, count, False, scratch),         # G = 65
               lambda: call(a, c0, keys, elts, out, -1, False, scratch),
               lambda: call(a, c0, keys, elts[:4] + [2], out, count, False, scratch),         # an even element
               lambda: call(a, c0, keys, elts[:4] + [2 << n_power], out, count, False, scratch),  # even once reduced
               lambda: call(None, c0, keys, elts, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, None, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [None], elts, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, out, count, False, None),
               lambda: call(a, c0, keys[:4], elts, out, count, False, scratch),               # one key per element
               lambda: call(a, c0, keys, elts, out, count, False, hoist_scratch(plan, count, G, short=1)),
               lambda: call(a, c0, keys, elts, out, count, False, off[8:]),                   # not 256-byte aligned
               lambda: call(a[1:], c0, keys, elts, out, count, False, scratch),               # too small
               lambda: call(a, c0[1:], keys, elts, out, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [keys[4][1:]], elts, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, out[1:], count, False, scratch),
               lambda: call(a.to(torch.int32), c0, keys, elts, out, count, False, scratch),
               # out or the scratch over a, c0, a key or each other
               lambda: call(tail[:a.numel()], c0, keys, elts, out, count, False, scratch),
               lambda: call(a, tail[-c0.numel():], keys, elts, out, count, False, scratch),
               lambda: call(a, c0, keys[:4] + [tail[:keys[0].numel()]], elts, out, count, False, scratch),
               lambda: call(a, c0, keys, elts, tail[-out.numel():], count, False, scratch),
               lambda: call(out[:a.numel()], c0, keys, elts, out, count, False, scratch),
               lambda: call(a, out[-c0.numel():], keys, elts, out, count, False, scratch),
               lambda: call(a, c0, [out[:keys[0].numel()]] + keys[1:], elts, out, count, False, scratch),
               lambda: bare.rotate_hoisted(a, c0, keys, elts, out, count, False, scratch)]    # no transforms
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    import torch
    n_power, L, K, alpha, G, count = 9, 3, 2, 2, 3, 2
    M, n = L + K, 1 << n_power
    st = ring(g, bits, n_power).sub(list(range(M)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    elts = elements_for(g, n_power, G)
    a, c0, keys = operands(g, plan, st, np.random.default_rng(0), count, G)
    out = filled(bits, G * 2 * count * L * n)
    scratch, scratch2 = hoist_scratch(plan, count, G), hoist_scratch(plan, count, G)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.rotate_hoisted(a, c0, keys, elts, out, count, True, scratch, stream=s)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.rotate_hoisted(a, c0, keys, elts, out, count, True, scratch, stream=s)
    for seed in (1, 2):
        na, nc0, nkeys = operands(g, plan, st, np.random.default_rng(seed), count, G)
        a.copy_(na), c0.copy_(nc0)
        for k, nk in zip(keys, nkeys):
            k.copy_(nk)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = filled(bits, G * 2 * count * L * n)
        plan.rotate_hoisted(a, c0, keys, elts, eager, count, True, scratch2)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed
        assert torch.equal(eager, composition(g, plan, st, a, c0, keys, elts, count, True)), seed


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_hoisted_rotation.cpp, compiled here against include/ and libgpuntt.so: three rotations of one
    ciphertext from one decompose, compared with the composition"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_hoisted_rotation")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_hoisted_rotation.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12",), ("10", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
