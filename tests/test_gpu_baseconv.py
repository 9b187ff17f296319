"""RNS fast base conversion on the MI355X (include/gpuntt/rns/base_conversion.cuh).  The expected values are a restatement
of the header's definitions in Python integers (ref_*, below): every output word of both modes and both calls for
small rings, what the outputs MEAN (the centred lift, the rounded division, rescale, the approximate overshoot),
sampled columns of the ring sizes the kernels are for, the composition with GPU_INTT / GPU_NTT, one launch per call,
hipGraph replay, a caller-owned workspace, argument checks and a C++ caller of the public header."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from gpu_utils import distinct_factors, find_ntt_factors
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LKS = [(1, 1), (1, 8), (3, 5), (8, 24), (17, 3), (64, 4), (4, 64)]
WIDTHS = {64: (62, 61, 60, 45, 20), 32: (30, 29, 20)}
COMPOSITES = {64: (15015, 215441, 47027 * 43, (2 ** 31 - 1) * (2 ** 29 - 3)), 32: (15015, 215441, 47027 * 43)}


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


_pools = {}


def moduli(bits, need):
    """`need` pairwise coprime moduli of mixed widths: NTT primes found by search, a few odd composites in between"""
    pool, used = _pools.setdefault(bits, ([], {}))
    while len(pool) < need:
        i = len(pool)
        if i % 9 == 4 and i // 9 < len(COMPOSITES[bits]):
            m = COMPOSITES[bits][i // 9]
        else:
            w = WIDTHS[bits][i % len(WIDTHS[bits])]
            m = find_ntt_factors(w, 3, skip=used.get(w, 0), clear_of_top=True)[0]
            used[w] = used.get(w, 0) + 1
        assert all(math.gcd(m, o) == 1 for o in pool), m
        pool.append(m)
    return pool[:need]


def bases(bits, L, K):
    """input and output base: the smaller one is spread evenly over the pool, so both mix every width"""
    ms = moduli(bits, L + K)
    small = min(L, K)
    pick = {ms[i * (L + K) // small] for i in range(small)}
    a, b = [m for m in ms if m in pick], [m for m in ms if m not in pick]
    return (a, b) if L <= K else (b, a)


# ---- the definitions, in Python integers (numpy object arrays: one Python int per word) ------------------------------
def ref_y(W, qs, x):
    """x: object array [count][L][N] of input words (any word value) -> y_i, canonical"""
    Q = math.prod(qs)
    return [(x[:, i, :] * pow(Q // q, -1, q)) % q for i, q in enumerate(qs)]


def ref_convert(W, qs, ps, x, centred):
    Q = math.prod(qs)
    y = ref_y(W, qs, x)
    v = 0
    if centred:
        zsum = 0
        for yi, q in zip(y, qs):
            b = q.bit_length()
            R = (1 << (W - 1 + b)) // q
            zsum = zsum + ((yi * R) >> (b - 1))
        v = (zsum + (1 << (W - 1))) >> W
    out = []
    for p in ps:
        s = 0
        for yi, q in zip(y, qs):
            s = s + yi * ((Q // q) % p)
        out.append((s - v * (Q % p)) % p)
    return np.stack(out, axis=1)  # [count][K][N]


def ref_divide(qs, ps, conv, c):
    Q = math.prod(qs)
    return np.stack([((c[:, j, :] - conv[:, j, :]) * pow(Q, -1, p)) % p for j, p in enumerate(ps)], axis=1)


def residues(values, ms):
    """object array [count][N] of integers -> [count][len(ms)][N] canonical residues"""
    return np.stack([values % m for m in ms], axis=1)


def random_words(rng, ms, count, n, bits, plant=True):
    """random canonical words [count][len(ms)][N] with planted 0, m - 1 and the non-canonical 2^W - 1"""
    x = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in ms]) for _ in range(count)])
    x = x.astype(object)
    if plant:
        for i, m in enumerate(ms):
            x[0, i, 0] = 0
            x[-1, i, n - 1] = m - 1
            x[(i + 1) % count, i, (3 * i + 1) % n] = (1 << bits) - 1
            x[i % count, i, (5 * i) % n] = m - 1
    return x


def dev(g, a, bits):
    return g.to_device(np.ascontiguousarray(a.astype(np.uint64)).astype(g.np_dtype(bits)).reshape(-1))


def host(g, t, shape):
    return g.to_host(t).astype(np.uint64).astype(object).reshape(shape)


def run(g, plan, bits, x, c, n_power, count, mode, alias=False):
    """one call on the GPU; returns the object array [count][K][N]"""
    import torch
    K = plan.out_count
    d_in = dev(g, x, bits)
    if c is None:
        d_out = torch.full((count * K << n_power,), -1, dtype=d_in.dtype, device=d_in.device)
        plan.convert(d_in, d_out, n_power, count, mode)
    else:
        d_c = dev(g, c, bits)
        d_out = d_c if alias else torch.full_like(d_c, -1)
        plan.convert_and_divide(d_in, d_c, d_out, n_power, count, mode)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(d_in).astype(np.uint64).astype(object).reshape(x.shape), x), "input modified"
    return host(g, d_out, (count, K, 1 << n_power))


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K", LKS)
@pytest.mark.parametrize("n_power", [1, 5, 12, 13])
def test_every_output_word(g, bits, L, K, n_power):
    """both modes, both calls, count = 3; out aliases c in half of the convert-and-divide cases"""
    qs, ps = bases(bits, L, K)
    plan = g.BaseConvPlan(qs, ps, bits)
    count, n = 3, 1 << n_power
    rng = np.random.default_rng(1000 * L + 10 * K + n_power + bits)
    x = random_words(rng, qs, count, n, bits)
    c = random_words(rng, ps, count, n, bits)
    case = LKS.index((L, K)) + n_power
    for mode in (g.APPROXIMATE, g.CENTRED):
        conv = ref_convert(bits, qs, ps, x, mode == g.CENTRED)
        got = run(g, plan, bits, x, None, n_power, count, mode)
        assert np.array_equal(got, conv), ("convert", mode)
        got = run(g, plan, bits, x, c, n_power, count, mode, alias=(case + mode) % 2 == 0)
        assert np.array_equal(got, ref_divide(qs, ps, conv, c)), ("convert_and_divide", mode)


def random_integers(rng, lo, hi, shape):
    """uniform Python integers in [lo, hi] as an object array (hi - lo may exceed 64 bits)"""
    span = hi - lo + 1
    limbs = (span.bit_length() + 62) // 62 + 1
    v = np.zeros(shape, dtype=object)
    for _ in range(limbs):
        v = (v << 62) + rng.integers(0, 1 << 62, size=shape, dtype=np.uint64).astype(object)
    return lo + v % span


MEANING = [(64, 3, 5), (64, 8, 24), (64, 64, 4), (64, 1, 8), (32, 5, 7), (32, 64, 3), (32, 4, 64)]


@pytest.mark.parametrize("bits,L,K", MEANING)
def test_centred_mode_returns_the_centred_value(g, bits, L, K):
    """integers |x| <= Q/2 - Q/2^20, given by their residues, come out as x mod p_j"""
    qs, ps = bases(bits, L, K)
    Q = math.prod(qs)
    n_power, count = 6, 2
    rng = np.random.default_rng(L * K)
    bound = Q // 2 - Q // (1 << 20)
    xs = random_integers(rng, -bound, bound, (count, 1 << n_power))
    xs[0, 0], xs[0, 1], xs[1, 0], xs[1, 1] = bound, -bound, 0, -1
    got = run(g, g.BaseConvPlan(qs, ps, bits), bits, residues(xs, qs), None, n_power, count, g.CENTRED)
    assert np.array_equal(got, residues(xs, ps))


def centred(r, Q):
    """the representative of r mod Q in [-Q/2, Q/2)"""
    r = r % Q
    return np.where((2 * r >= Q).astype(bool), r - Q, r)


@pytest.mark.parametrize("bits,L,K", MEANING)
def test_convert_and_divide_is_the_rounded_division(g, bits, L, K):
    """C in the base q u p, away from the band: (C - centred(C mod Q)) // Q mod p_j"""
    qs, ps = bases(bits, L, K)
    Q, P = math.prod(qs), math.prod(ps)
    n_power, count = 6, 2
    rng = np.random.default_rng(L + K)
    bound = Q // 2 - Q // (1 << 20)
    C = random_integers(rng, 0, P - 1, (count, 1 << n_power)) * Q + random_integers(rng, -bound, bound,
                                                                                     (count, 1 << n_power))
    C = C % (Q * P)
    want = residues((C - centred(C, Q)) // Q, ps)
    got = run(g, g.BaseConvPlan(qs, ps, bits), bits, residues(C, qs), residues(C, ps), n_power, count, g.CENTRED)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits,K", [(64, 31), (64, 1), (32, 8)])
def test_rescale_is_the_one_modulus_case(g, bits, K):
    """rescale: drop the last prime q of the base p u {q} and divide by it, rounding -- L = 1"""
    ms = moduli(bits, K + 1)
    q, ps = ms[K], ms[:K]
    n_power, count = 7, 2
    rng = np.random.default_rng(K)
    C = random_integers(rng, 0, q * math.prod(ps) - 1, (count, 1 << n_power))
    r = C % q
    away = (2 * r < q) | (2 * r >= q + 8)  # the band [q/2, q/2 + 3 q / 2^W) holds at most 3 values
    C = np.where(away.astype(bool), C, C - r)
    want = residues((C - centred(C, q)) // q, ps)  # = round(C / q)
    assert np.array_equal(want, residues((2 * C + q) // (2 * q), ps))
    got = run(g, g.BaseConvPlan([q], ps, bits), bits, residues(C, [q]), residues(C, ps), n_power, count, g.CENTRED)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits,L,K", MEANING)
def test_approximate_mode_overshoots_by_less_than_L_times_Q(g, bits, L, K):
    """out = (x~ + u Q) mod p_j with one u in [0, L) for the whole column"""
    qs, ps = bases(bits, L, K)
    Q = math.prod(qs)
    n_power, count = 5, 2
    rng = np.random.default_rng(7 * L + K)
    xs = random_integers(rng, 0, Q - 1, (count, 1 << n_power))
    got = run(g, g.BaseConvPlan(qs, ps, bits), bits, residues(xs, qs), None, n_power, count, g.APPROXIMATE)
    found = np.zeros(xs.shape, dtype=bool)
    for u in range(L):
        found |= np.all((got == residues(xs + u * Q, ps)).astype(bool), axis=1)
    assert found.all()


def sampled_columns(g, n, rng):
    """at least 2048 columns: the first and last 64, both sides of every workgroup-tile boundary, random ones"""
    tile = g.BASECONV_TILE
    edges = np.arange(tile, n, tile)
    cols = np.concatenate([np.arange(64), np.arange(n - 64, n), edges - 1, edges, rng.integers(0, n, size=2048)])
    return np.unique(cols)


@pytest.mark.parametrize("bits,L,K,n_power,count", [(64, 8, 24, 16, 4), (64, 64, 4, 16, 1), (64, 3, 5, 20, 1),
                                                    (32, 8, 8, 16, 4)])
def test_ring_sizes_the_kernels_are_for(g, bits, L, K, n_power, count):
    import torch
    qs, ps = bases(bits, L, K)
    plan = g.BaseConvPlan(qs, ps, bits)
    n = 1 << n_power
    rng = np.random.default_rng(n_power + L)
    x = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in qs]) for _ in range(count)])
    c = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in ps]) for _ in range(count)])
    x[:, :, ::4099] = (1 << bits) - 1
    d_x, d_c = g.to_device(x.astype(g.np_dtype(bits)).reshape(-1)), g.to_device(c.astype(g.np_dtype(bits)).reshape(-1))
    d_conv, d_div = torch.full_like(d_c, -1), torch.full_like(d_c, -1)
    plan.convert(d_x, d_conv, n_power, count, g.APPROXIMATE)
    plan.convert_and_divide(d_x, d_c, d_div, n_power, count, g.CENTRED)
    torch.cuda.synchronize()
    got_conv = g.to_host(d_conv).astype(np.uint64).reshape(count, K, n)
    got_div = g.to_host(d_div).astype(np.uint64).reshape(count, K, n)
    for e in range(count):
        cols = sampled_columns(g, n, rng)
        assert cols.size >= 2048
        xe, ce = x[e:e + 1][:, :, cols].astype(object), c[e:e + 1][:, :, cols].astype(object)
        assert np.array_equal(got_conv[e:e + 1][:, :, cols].astype(object), ref_convert(bits, qs, ps, xe, False))
        want = ref_divide(qs, ps, ref_convert(bits, qs, ps, xe, True), ce)
        assert np.array_equal(got_div[e:e + 1][:, :, cols].astype(object), want)


def test_composition_with_the_transforms(g):
    """base q, NTT form --GPU_INTT (RNS)--> coefficients --convert (centred)--> base p --GPU_NTT (RNS)--> must be the
    oracle's NTT of the centred-lifted polynomial"""
    import torch
    from gpu_utils import MergeCase
    logn, poly, L, K = 12, O.X_N_plus, 3, 4
    n = 1 << logn
    cases = [MergeCase(g, 64, logn, poly, f) for f in distinct_factors((60, 59, 58, 60, 59, 57, 56), logn)]
    cq, cp = cases[:L], cases[L:]
    qs, ps = [c.q for c in cq], [c.q for c in cp]
    Q = math.prod(qs)

    def stack(cs):
        fwd = np.zeros(len(cs) * n, dtype=np.uint64)
        inv = np.zeros_like(fwd)
        for i, c in enumerate(cs):
            fwd[i * n:i * n + c.prm.root_of_unity_size] = c.prm.forward_table_device_order
            inv[i * n:i * n + c.prm.root_of_unity_size] = c.prm.inverse_table_device_order
        return (g.to_device(fwd), g.to_device(inv), g.modulus_array_to_device([c.prm.modulus for c in cs], 64),
                g.to_device(np.array([c.prm.n_inv for c in cs], dtype=np.uint64)))

    _, inv_q, mods_q, ninv_q = stack(cq)
    fwd_p, _, mods_p, _ = stack(cp)
    count = 2
    X = np.concatenate([cq[r % L].random(1, seed=40 + r) for r in range(count * L)])
    # host: the coefficients (oracle INTT), lifted to the centred integer by the CRT
    coef = np.stack([cq[r % L].P.merge_ntt(X[r * n:(r + 1) * n], cq[r % L].oprm, inverse=True)
                     for r in range(count * L)]).astype(object).reshape(count, L, n)
    lifted = sum(coef[:, i, :] * (Q // q) * pow(Q // q, -1, q) for i, q in enumerate(qs)) % Q
    assert not np.any((2 * lifted >= Q) & (2 * lifted < Q + Q // (1 << 50))), "a coefficient inside the band"
    lifted = centred(lifted, Q)
    want = np.stack([cp[j].P.merge_ntt((lifted[e] % ps[j]).astype(np.uint64), cp[j].oprm)
                     for e in range(count) for j in range(K)]).reshape(-1)

    d_X = g.to_device(X)
    d_coef = torch.zeros_like(d_X)
    g.GPU_INTT(d_X, d_coef, inv_q, mods_q,
               g.ntt_rns_configuration(n_power=logn, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=ninv_q),
               count * L, L)
    d_p = torch.zeros(count * K * n, dtype=d_X.dtype, device=d_X.device)
    g.BaseConvPlan(qs, ps, 64).convert(d_coef, d_p, logn, count, g.CENTRED)
    d_out = torch.zeros_like(d_p)
    g.GPU_NTT(d_p, d_out, fwd_p, mods_p, g.ntt_rns_configuration(n_power=logn, reduction_poly=poly), count * K, K)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(d_out), want)


@pytest.mark.parametrize("L,K", [(1, 1), (8, 24), (64, 64)])
def test_one_launch_per_call(g, L, K):
    import torch
    qs, ps = bases(64, L, K)
    plan = g.BaseConvPlan(qs, ps, 64)
    for n_power, count in ((5, 1), (13, 3)):
        d_in = torch.zeros(count * L << n_power, dtype=torch.int64, device="cuda:0")
        d_c = torch.zeros(count * K << n_power, dtype=torch.int64, device="cuda:0")
        d_out = torch.zeros_like(d_c)
        for mode in (g.APPROXIMATE, g.CENTRED):
            with g.launch_log() as log:
                plan.convert(d_in, d_out, n_power, count, mode)
            assert len(log.kernels) == 1 and log.kernels[0].startswith("base_convert"), log.kernels
            with g.launch_log() as log:
                plan.convert_and_divide(d_in, d_c, d_out, n_power, count, mode)
            assert len(log.kernels) == 1 and log.kernels[0].startswith("base_convert"), log.kernels
    torch.cuda.synchronize()


def test_graph_capture_and_replay_with_new_data(g):
    import torch
    bits, L, K, n_power, count = 64, 8, 24, 10, 3
    qs, ps = bases(bits, L, K)
    plan = g.BaseConvPlan(qs, ps, bits)
    n = 1 << n_power
    d_in = torch.zeros(count * L * n, dtype=torch.int64, device="cuda:0")
    d_c = torch.zeros(count * K * n, dtype=torch.int64, device="cuda:0")
    d_up, d_down = torch.zeros_like(d_c), torch.zeros_like(d_c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.convert(d_in, d_up, n_power, count, g.APPROXIMATE)
        plan.convert_and_divide(d_in, d_c, d_down, n_power, count, g.CENTRED)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.convert(d_in, d_up, n_power, count, g.APPROXIMATE)
        plan.convert_and_divide(d_in, d_c, d_down, n_power, count, g.CENTRED)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        x, c = random_words(rng, qs, count, n, bits), random_words(rng, ps, count, n, bits)
        d_in.copy_(dev(g, x, bits))
        d_c.copy_(dev(g, c, bits))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(g, d_up, (count, K, n)), ref_convert(bits, qs, ps, x, False))
        assert np.array_equal(host(g, d_down, (count, K, n)),
                              ref_divide(qs, ps, ref_convert(bits, qs, ps, x, True), c))


def test_caller_owned_workspace_allocates_nothing(g):
    import torch
    bits, L, K, n_power, count = 64, 8, 24, 8, 2
    qs, ps = bases(bits, L, K)
    n = 1 << n_power
    rng = np.random.default_rng(3)
    x = random_words(rng, qs, count, n, bits)
    d_in = dev(g, x, bits)
    d_out = torch.zeros(count * K * n, dtype=torch.int64, device="cuda:0")
    ws = torch.zeros(g.BaseConvPlan.workspace_bytes(L, K, bits), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    plan = g.BaseConvPlan(qs, ps, bits, workspace=ws)
    plan.convert(d_in, d_out, n_power, count, g.CENTRED)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert not plan.owns_workspace  # the API's own accounting: nothing was allocated outside torch's allocator either
    assert np.array_equal(host(g, d_out, (count, K, n)), ref_convert(bits, qs, ps, x, True))
    assert g.BaseConvPlan(qs, ps, bits).owns_workspace
    with pytest.raises(ValueError):
        g.BaseConvPlan(qs, ps, bits, workspace=ws[:64])


def test_bad_arguments_are_refused_before_any_launch(g):
    import torch
    bits, L, K, n_power, count = 64, 3, 5, 6, 2
    qs, ps = bases(bits, L, K)
    plan = g.BaseConvPlan(qs, ps, bits)
    n = 1 << n_power
    buf = torch.zeros(count * (L + 2 * K) * n, dtype=torch.int64, device="cuda:0")
    d_in, d_c, d_out = buf[:count * L * n], buf[count * L * n:count * (L + K) * n], buf[count * (L + K) * n:]
    calls = [
        lambda: plan.convert(d_in, d_out, 0, count),
        lambda: plan.convert(d_in, d_out, 29, count),
        lambda: plan.convert(d_in, d_out, n_power, -1),
        lambda: plan.convert(d_in, d_out, n_power, count, mode=2),
        lambda: plan.convert(d_in, d_in, n_power, 1),                       # aliased
        lambda: plan.convert(buf, buf[n:], n_power, count),                 # overlapping
        lambda: plan.convert(d_in[1:], d_out, n_power, count),              # in short
        lambda: plan.convert_and_divide(d_in, d_c, d_out[1:], n_power, count),  # out short
        lambda: plan.convert_and_divide(d_in, d_c[1:], d_out, n_power, count),  # c short
        lambda: plan.convert(d_in.to(torch.int32), d_out, n_power, count),  # wrong width
    ]
    for call in calls:
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                call()
        assert log.kernels == []
    torch.cuda.synchronize()


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_baseconv.cpp, compiled here against include/ and libgpuntt.so: a ModUp, then a ModDown back,
    every word checked against host integers"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_baseconv")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "example_baseconv.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12", "3"), ("14", "2", "u32")):
            r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
