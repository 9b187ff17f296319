"""RNS inner product on the MI355X (include/gpuntt/rns/inner_product.cuh).  Expected values are the header's definition
restated in Python integers (innerprod_utils.ref_inner_product) for small cases and the library's host reference --
pinned to Python integers by tests/test_inner_product_host.py -- for larger ones; every comparison is exact equality of
every output word.  Then: the one-word path through an offset base pointer, the reference-pinned oracle (pointwise
product, ring products through the transforms), the ring sizes the kernel is for, one launch per call, hipGraph
replay, a caller-owned workspace, count = 0, argument checks and a C++ caller of the public header."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from gpu_utils import MergeCase, distinct_factors_scaled
from innerprod_utils import from_words, moduli, operands, ref_inner_product, words
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYTHON_INTEGER_LIMIT = 1 << 19  # products above which the expected values come from the host reference


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def expected(g, bits, qs, a, key, out0, n_power, D, count, limbs, accumulate, key_mod_count):
    C = key.shape[1]
    if D * C * count * len(qs) << n_power <= PYTHON_INTEGER_LIMIT:
        return ref_inner_product(qs, a, key, out0, D, limbs, accumulate)
    out = words(g, out0, bits)
    g.innerprod_reference(qs, words(g, a, bits), words(g, key, bits), out, n_power, D, C, count, accumulate,
                          key_mod_count, limbs, bits)
    return from_words(out, out0.shape)


def run(g, plan, bits, a, key, out0, n_power, D, count, limbs, accumulate, key_mod_count, offset=0):
    """one call on the GPU; returns the object array [C][count][M][N].  offset: words by which every base pointer is
    moved off its 16-byte alignment"""
    import torch
    C = key.shape[1]

    def dev(x, fill=None):
        w = words(g, x, bits)
        t = torch.zeros(w.size + offset, dtype=torch.int64 if bits == 64 else torch.int32, device="cuda:0")
        t[offset:] = g.to_device(w) if fill is None else fill
        return t[offset:]

    d_a, d_key = dev(a), dev(key)
    d_out = dev(out0) if accumulate else dev(out0, fill=-1)  # an unwritten word shows
    assert all(t.data_ptr() % 16 == (offset * bits // 8) % 16 for t in (d_a, d_key, d_out))
    plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, accumulate, key_mod_count, limbs)
    torch.cuda.synchronize()
    assert np.array_equal(from_words(g.to_host(d_a), a.shape), a), "a modified"
    assert np.array_equal(from_words(g.to_host(d_key), key.shape), key), "key modified"
    return from_words(g.to_host(d_out), out0.shape)


def check(g, bits, n_power, D, C, count, M, seed, offset=0):
    """both uses of one shape: accumulate off with the identity limbs, accumulate on with permuted limbs; in both the
    key has more limbs and more digits than the call uses"""
    qs = moduli(bits, 13)[seed % 5:][:M]
    plan = g.InnerProductPlan(qs, bits)
    rng = np.random.default_rng(seed)
    km = M + 3
    perm = [int(v) for v in rng.permutation(km)[:M]]
    a, key, out0 = operands(rng, bits, qs, n_power, D, C, count, D + 1, km)
    for limbs, accumulate in ((None, False), (perm, True)):
        want = expected(g, bits, qs, a, key, out0, n_power, D, count, limbs, accumulate, km)
        got = run(g, plan, bits, a, key, out0, n_power, D, count, limbs, accumulate, km, offset)
        assert np.array_equal(got, want), (limbs, accumulate)


# every value of every axis, and every (components, inputs per block) form of the kernel: n_power, D, C, count, M
SHAPES = [(1, 1, 1, 1, 1), (1, 64, 4, 5, 3), (2, 2, 2, 2, 8), (2, 17, 3, 1, 3), (5, 16, 4, 2, 3), (5, 64, 2, 5, 8),
          (9, 1, 2, 1, 8), (9, 17, 1, 5, 3), (9, 2, 3, 2, 1), (9, 16, 4, 5, 1), (9, 64, 2, 2, 3), (2, 64, 1, 2, 8)]
SHAPES += [(5, 3, C, count, 3) for C, count in itertools.product((1, 2, 3, 4), (1, 2, 5))]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power,D,C,count,M", SHAPES)
def test_every_output_word(g, bits, n_power, D, C, count, M):
    check(g, bits, n_power, D, C, count, M, seed=1000 * n_power + 10 * D + C + count + M + bits)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("C,count", [(4, 2), (2, 5), (1, 1)])
def test_the_largest_sum_the_contract_allows(g, bits, C, count):
    """D = 64, every word of a and the key 2^W - 1, out prefilled with 2^W - 1, accumulating: moduli of every width"""
    qs = moduli(bits, 8)
    top, D, n_power, M = (1 << bits) - 1, 64, 5, 8
    n = 1 << n_power
    a = np.full((D, count, M, n), top, dtype=object)
    key = np.full((D, C, M, n), top, dtype=object)
    out0 = np.full((C, count, M, n), top, dtype=object)
    got = run(g, g.InnerProductPlan(qs, bits), bits, a, key, out0, n_power, D, count, None, True, M)
    for m, q in enumerate(qs):
        assert (got[:, :, m, :] == (top + 64 * top * top) % q).all(), q


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("C,count", [(1, 5), (2, 1), (3, 2), (4, 5)])
def test_a_base_pointer_offset_by_one_word_takes_the_one_word_path(g, bits, C, count):
    """the same operands at 16-byte aligned and at odd-word base pointers: both equal the definition, hence each other"""
    for offset in (0, 1):
        check(g, bits, 6, 3, C, count, 3, seed=77 + C + count, offset=offset)


@pytest.mark.parametrize("bits", [64, 32])
def test_hadamard_product_equals_the_oracle_pointwise(g, bits):
    """D = 1, C = 1, count = batch on canonical inputs: the oracle's pointwise (the reference's NTTCPU::mult)"""
    P = O.Port(bits)
    logn, batch = 10, 3
    mod = P.merge_params(logn, O.X_N_plus)["mod"]
    q, n = mod[0], 1 << logn
    a, key = P.splitmix(5, 0, batch * n, q), P.splitmix(6, 0, n, q)
    want = np.concatenate([P.pointwise(a[r * n:(r + 1) * n], key, mod) for r in range(batch)])
    got = run(g, g.InnerProductPlan([q], bits), bits, a.astype(object).reshape(1, batch, 1, n),
              key.astype(object).reshape(1, 1, 1, n), np.zeros((1, batch, 1, n), dtype=object), logn, 1, batch, None,
              False, 1)
    assert np.array_equal(got.reshape(-1), want.astype(object))


@pytest.mark.parametrize("logn", [5, 10])
def test_ring_products_through_the_transforms(g, logn):
    """negacyclic, D = 3, two moduli: GPU_INTT(inner(GPU_NTT(a), GPU_NTT(k))) is the sum over d of the oracle's
    ntt / pointwise / intt ring products"""
    import torch
    D, M, poly, n = 3, 2, O.X_N_plus, 1 << logn
    cases = [MergeCase(g, 64, logn, poly, f) for f in distinct_factors_scaled((60, 59), logn)]
    qs = [c.q for c in cases]
    fwd, inv = np.zeros(M * n, dtype=np.uint64), np.zeros(M * n, dtype=np.uint64)
    for i, c in enumerate(cases):
        fwd[i * n:i * n + c.prm.root_of_unity_size] = c.prm.forward_table_device_order
        inv[i * n:i * n + c.prm.root_of_unity_size] = c.prm.inverse_table_device_order
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], 64)
    ninv = g.to_device(np.array([c.prm.n_inv for c in cases], dtype=np.uint64))
    a = np.concatenate([cases[p % M].random(1, seed=10 + p) for p in range(D * M)])  # [D][1][M][N]
    k = np.concatenate([cases[p % M].random(1, seed=50 + p) for p in range(D * M)])  # [D][1][M][N]
    want = np.zeros((M, n), dtype=object)
    for d in range(D):
        for m, c in enumerate(cases):
            at = (d * M + m) * n
            fa, fk = c.P.merge_ntt(a[at:at + n], c.oprm), c.P.merge_ntt(k[at:at + n], c.oprm)
            prod = c.P.merge_ntt(c.P.pointwise(fa, fk, c.oprm["mod"]), c.oprm, inverse=True)
            want[m] = (want[m] + prod.astype(object)) % c.q
    d_a, d_k = g.to_device(a), g.to_device(k)
    cfg = g.ntt_rns_configuration(n_power=logn, reduction_poly=poly)
    g.GPU_NTT_Inplace(d_a, g.to_device(fwd), mods, cfg, D * M, M)
    g.GPU_NTT_Inplace(d_k, g.to_device(fwd), mods, cfg, D * M, M)
    d_out = torch.full((M * n,), -1, dtype=torch.int64, device="cuda:0")
    g.InnerProductPlan(qs, 64).multiply_accumulate(d_a, d_k, d_out, logn, D, 1, 1)
    g.GPU_INTT_Inplace(d_out, g.to_device(inv), mods,
                       g.ntt_rns_configuration(n_power=logn, ntt_type=g.INVERSE, reduction_poly=poly, mod_inverse=ninv),
                       M, M)
    torch.cuda.synchronize()
    assert np.array_equal(from_words(g.to_host(d_out), (M, n)), want)


@pytest.mark.parametrize("bits,n_power,M,D,C,count", [(64, 16, 8, 3, 2, 2), (32, 14, 4, 4, 2, 3)])
def test_ring_sizes_the_kernel_is_for(g, bits, n_power, M, D, C, count):
    """against the host reference: accumulate off into a -1 prefill, then accumulate on through permuted limbs of a
    key with two more limbs and one more digit"""
    import torch
    qs = moduli(bits, M)
    plan = g.InnerProductPlan(qs, bits)
    n, km, dt = 1 << n_power, M + 2, g.np_dtype(bits)
    rng = np.random.default_rng(n_power + M)
    top = np.iinfo(dt).max
    a = rng.integers(0, top, size=D * count * M * n, dtype=dt, endpoint=True)
    key = rng.integers(0, top, size=(D + 1) * C * km * n, dtype=dt, endpoint=True)
    a[::4099], key[::4001] = top, top
    limbs = [int(v) for v in rng.permutation(km)[:M]]
    want = np.zeros(C * count * M * n, dtype=dt)
    g.innerprod_reference(qs, a, key, want, n_power, D, C, count, False, km, None, bits)
    d_a, d_key = g.to_device(a), g.to_device(key)
    d_out = torch.full((want.size,), -1, dtype=d_a.dtype, device="cuda:0")
    plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, False, km)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(d_out), want)
    g.innerprod_reference(qs, a, key, want, n_power, D, C, count, True, km, limbs, bits)
    plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, True, km, limbs)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(d_out), want)
    assert np.array_equal(g.to_host(d_a), a) and np.array_equal(g.to_host(d_key), key)


def test_one_launch_per_call_and_none_for_count_zero(g):
    import torch
    M, D, C = 3, 3, 2
    plan = g.InnerProductPlan(moduli(64, M), 64)
    families = set()
    for n_power, count in ((5, 1), (13, 5)):
        d_a = torch.zeros(D * count * M << n_power, dtype=torch.int64, device="cuda:0")
        d_key = torch.zeros(D * C * (M + 1) << n_power, dtype=torch.int64, device="cuda:0")
        d_out = torch.full((C * count * M << n_power,), -1, dtype=torch.int64, device="cuda:0")
        for accumulate, limbs in itertools.product((False, True), (None, [3, 0, 1])):
            with g.launch_log() as log:
                plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, accumulate, M + 1, limbs)
            assert len(log.kernels) == 1, log.kernels
            families.add(log.kernels[0])
        with g.launch_log() as log:
            plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, 0, False, M + 1)
        assert log.kernels == []
    torch.cuda.synchronize()
    assert families == {"inner_product"}  # the same kernel family with and without key_limbs


def test_graph_capture_and_replay_with_new_data(g):
    import torch
    bits, M, D, C, count, n_power = 64, 3, 3, 2, 5, 8
    qs = moduli(bits, M)
    plan = g.InnerProductPlan(qs, bits)
    km, limbs = M + 1, [3, 1, 0]
    n = 1 << n_power
    d_a = torch.zeros(D * count * M * n, dtype=torch.int64, device="cuda:0")
    d_key = torch.zeros(D * C * km * n, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(C * count * M * n, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, False, km, limbs)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count, False, km, limbs)
    limbs[0] = 2  # the indices travelled with the captured launch: the caller's list is free again
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        a, key, out0 = operands(rng, bits, qs, n_power, D, C, count, D, km)
        d_a.copy_(g.to_device(words(g, a, bits)))
        d_key.copy_(g.to_device(words(g, key, bits)))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(from_words(g.to_host(d_out), out0.shape),
                              ref_inner_product(qs, a, key, out0, D, [3, 1, 0], False))


def test_caller_owned_workspace_allocates_nothing(g):
    import torch
    bits, M, D, C, count, n_power = 64, 8, 2, 2, 2, 6
    qs = moduli(bits, M)
    rng = np.random.default_rng(3)
    a, key, out0 = operands(rng, bits, qs, n_power, D, C, count, D, M)
    d_a, d_key = g.to_device(words(g, a, bits)), g.to_device(words(g, key, bits))
    d_out = torch.zeros(out0.size, dtype=torch.int64, device="cuda:0")
    ws = torch.zeros(g.InnerProductPlan.workspace_bytes(M, bits), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    plan = g.InnerProductPlan(qs, bits, workspace=ws)
    plan.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert not plan.owns_workspace
    want = ref_inner_product(qs, a, key, out0, D)
    assert np.array_equal(from_words(g.to_host(d_out), out0.shape), want)
    own = g.InnerProductPlan(qs, bits)
    assert own.owns_workspace
    d_out.fill_(-1)
    own.multiply_accumulate(d_a, d_key, d_out, n_power, D, C, count)
    torch.cuda.synchronize()
    assert np.array_equal(from_words(g.to_host(d_out), out0.shape), want)
    with pytest.raises(ValueError):
        g.InnerProductPlan(qs, bits, workspace=ws[:64])


def test_bad_arguments_are_refused_before_any_launch(g):
    import torch
    bits, M, D, C, count, n_power, km = 64, 3, 2, 2, 2, 6, 4
    plan = g.InnerProductPlan(moduli(bits, M), bits)
    n = 1 << n_power
    sizes = [D * count * M * n, D * C * km * n, C * count * M * n]
    buf = torch.zeros(sum(sizes), dtype=torch.int64, device="cuda:0")
    d_a, d_key, d_out = torch.split(buf, sizes)

    def call(a=d_a, key=d_key, out=d_out, n_power=n_power, D=D, C=C, count=count, km=km, limbs=None):
        plan.multiply_accumulate(a, key, out, n_power, D, C, count, False, km, limbs)

    refused = [
        dict(n_power=0), dict(n_power=29), dict(D=0), dict(D=65), dict(C=0), dict(C=5), dict(count=-1),
        dict(km=M - 1), dict(km=257), dict(limbs=[0, 4, 1]), dict(limbs=[0, -1, 1]), dict(limbs=[0, 1]),
        dict(out=d_a), dict(out=d_key), dict(out=buf[n:]), dict(out=buf[sizes[0] + sizes[1] - 1:]),  # overlaps
        dict(a=d_a[1:]), dict(key=d_key[1:]), dict(out=d_out[1:]),                                   # short
        dict(a=d_a.to(torch.int32)), dict(out=d_out.to(torch.float64)),                              # wrong type
    ]
    for kw in refused:
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                call(**kw)
        assert log.kernels == [], kw
    with g.launch_log() as log:
        call()
    assert log.kernels == ["inner_product"]
    torch.cuda.synchronize()


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_inner_product.cpp, compiled here against include/ and libgpuntt.so: a small key switch (ModUp,
    GPU_NTT, inner product, GPU_INTT, ModDown) with the inner product checked against InnerProductPlan::reference"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_inner_product")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_inner_product.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("12", "3"), ("10", "2", "u32")):
            r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
