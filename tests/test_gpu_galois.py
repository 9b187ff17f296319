"""Galois automorphisms on the MI355X (include/gpuntt/ntt_merge/galois.cuh): the NTT-domain permutation of GPU_NTT's
output against the oracle's NTTCPU of numpy sigma_k(x), the coefficient domain (single modulus and RNS stacks) against
numpy sigma_k, the round trip through GPU_INTT, large rings with sampled checks, one launch per call, hipGraph capture,
argument checks, and a C++ caller of the public header."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from gpu_utils import MergeCase, rns_stack
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGNS = [1, 2, 5, 10, 12, 13, 14, 15, 16, 17, 20]


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def sigma(x, k, poly, q):
    """numpy sigma_k on the last axis; q is a scalar or one modulus per row"""
    x = np.asarray(x, dtype=np.uint64)
    n = x.shape[-1]
    j = np.arange(n, dtype=np.int64)
    out = np.empty_like(x)
    if poly == O.X_N_plus:
        e = (k * j) % (2 * n)
        qq = np.asarray(q, dtype=np.uint64).reshape(-1, 1) if np.ndim(q) else np.uint64(q)
        out[..., e % n] = np.where(e >= n, (qq - x) % qq, x)
    else:
        out[..., (k * j) % n] = x
    return out


def case_params(logn, idx):
    """a batch that is a multiple of nothing convenient and G in {1, 3, 8}, rotating through the grid"""
    batch = 7 if logn <= 13 else (3 if logn <= 17 else 1)
    G = (1, 3, 8)[idx % 3]
    two_n = 2 << logn
    ks = [pow(5, r, two_n) for r in (1, -1, 2, 3, -5, 7, 11)][:G - 1] + [two_n - 1]
    return batch, ks


def as_host(g, t, bits):
    return g.to_host(t).astype(np.uint64) if bits == 32 else g.to_host(t)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", LOGNS)
def test_ntt_domain_against_oracle(g, bits, poly, logn):
    import torch
    c = MergeCase(g, bits, logn, poly)
    batch, ks = case_params(logn, LOGNS.index(logn) + poly)
    x = c.random(batch, seed=77 + logn)
    d_x = g.to_device(x)
    d_y = torch.zeros_like(d_x)
    g.GPU_NTT(d_x, d_y, c.fwd_dev, c.prm.modulus, c.cfg(), batch)
    d_out = torch.full((len(ks) * batch * c.n,), -1, dtype=d_x.dtype, device=d_x.device)
    g.GPU_Automorphism_NTT(d_y, d_out, ks, logn, poly, batch)
    torch.cuda.synchronize()
    got = g.to_host(d_out).reshape(len(ks), batch, c.n)
    xs = x.reshape(batch, c.n)
    for gi, k in enumerate(ks):
        want = c.P.merge_ntt(sigma(xs, k, poly, c.q).astype(c.P.T), c.oprm).reshape(batch, c.n)
        assert np.array_equal(got[gi], want), (k, gi)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", LOGNS)
def test_coefficient_domain_single_modulus(g, bits, poly, logn):
    import torch
    c = MergeCase(g, bits, logn, poly)
    batch, ks = case_params(logn, LOGNS.index(logn) + 1)
    x = c.random(batch, seed=5 + logn)
    x[:: max(1, x.size // 17)] = 0  # zeros stay zero under the negation
    d_x = g.to_device(x)
    d_out = torch.full((len(ks) * batch * c.n,), -1, dtype=d_x.dtype, device=d_x.device)
    g.GPU_Automorphism(d_x, d_out, ks, c.prm.modulus, logn, poly, batch)
    torch.cuda.synchronize()
    got = as_host(g, d_out, bits).reshape(len(ks), batch, c.n)
    for gi, k in enumerate(ks):
        assert np.array_equal(got[gi], sigma(x.reshape(batch, c.n), k, poly, c.q)), (k, gi)


@pytest.mark.parametrize("bits,widths", [(64, (61, 62, 50)), (64, (55, 60)), (32, (30, 28, 29))])
@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", [1, 5, 12, 13, 14, 16, 17])
def test_coefficient_domain_rns(g, bits, widths, poly, logn):
    import torch
    cases, _, _ = rns_stack(g, bits, logn, widths, poly)
    mc, n = len(cases), 1 << logn
    batch = 2 * mc + 1
    _, ks = case_params(logn, logn)
    qs = np.array([cases[p % mc].q for p in range(batch)], dtype=np.uint64)
    x = np.concatenate([cases[p % mc].random(1, seed=100 + p) for p in range(batch)]).astype(np.uint64)
    mods = g.modulus_array_to_device([c.prm.modulus for c in cases], bits)
    d_x = g.to_device(x.astype(np.uint32) if bits == 32 else x)
    d_out = torch.full((len(ks) * batch * n,), -1, dtype=d_x.dtype, device=d_x.device)
    g.GPU_Automorphism(d_x, d_out, ks, mods, logn, poly, batch, mod_count=mc)
    torch.cuda.synchronize()
    got = as_host(g, d_out, bits).reshape(len(ks), batch, n)
    for gi, k in enumerate(ks):
        assert np.array_equal(got[gi], sigma(x.reshape(batch, n), k, poly, qs)), (k, gi)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", [3, 12, 16])
def test_round_trip_through_the_inverse_transform(g, bits, poly, logn):
    """INTT(Automorphism_NTT(NTT(x))) == Automorphism(x), all on the GPU"""
    import torch
    c = MergeCase(g, bits, logn, poly)
    batch, ks = 5, [g.galois_element_for_rotation(3, logn), g.galois_element_for_conjugation(logn)]
    x = c.random(batch, seed=9)
    d_x = g.to_device(x)
    d_y = torch.zeros_like(d_x)
    g.GPU_NTT(d_x, d_y, c.fwd_dev, c.prm.modulus, c.cfg(), batch)
    d_rot = torch.zeros(len(ks) * batch * c.n, dtype=d_x.dtype, device=d_x.device)
    g.GPU_Automorphism_NTT(d_y, d_rot, ks, logn, poly, batch)
    d_back = torch.zeros_like(d_rot)
    g.GPU_INTT(d_rot, d_back, c.inv_dev, c.prm.modulus, c.cfg(True), batch * len(ks))
    d_coef = torch.zeros_like(d_rot)
    g.GPU_Automorphism(d_x, d_coef, ks, c.prm.modulus, logn, poly, batch)
    torch.cuda.synchronize()
    assert torch.equal(d_back, d_coef)


def _brev(v, bits):
    r = np.zeros_like(v)
    for b in range(bits):
        r |= ((v >> b) & 1) << (bits - 1 - b)
    return r


def _closed_form_source(i, k, logn, poly, coefficient):
    """the source of output slot / coefficient i from the formulas in galois.cuh, evaluated in numpy (independent of the
    library's index functions); coefficient X_N_plus: j >= N means -in[j - N]"""
    n = 1 << logn
    if coefficient:
        mod = 2 * n if poly == O.X_N_plus else n
        return (pow(int(k), -1, mod) * i) % mod
    if poly == O.X_N_plus:
        e = (int(k) % (2 * n)) * (2 * _brev(i, logn) + 1) % (2 * n)
        return _brev((e - 1) // 2, logn)
    return _brev((int(k) % n) * _brev(i, logn) % n, logn)


def _sampled_check(g, d_in, d_out, ks, logn, poly, batch, q=None, samples=1 << 20):
    """compare 2^20 output words -- random ones, plus the last 2^16 of the output, where the offsets are largest -- with
    the input words the closed-form formula names, on the device"""
    import torch
    n = 1 << logn
    total = len(ks) * batch * n
    rng = np.random.default_rng(logn)
    flat = np.concatenate([rng.integers(0, total, size=samples - (1 << 16), dtype=np.int64),
                           np.arange(total - (1 << 16), total, dtype=np.int64)])
    gi, p, i = flat // (batch * n), (flat // n) % batch, flat % n
    src = np.empty(samples, dtype=np.int64)
    neg = np.zeros(samples, dtype=bool)
    for e, k in enumerate(ks):
        sel = gi == e
        j = _closed_form_source(i[sel], k, logn, poly, q is not None)
        neg[sel] = j >= n
        src[sel] = p[sel] * n + (j % n)
    dev = d_in.device
    got = d_out.index_select(0, torch.from_numpy(flat).to(dev))
    want = d_in.index_select(0, torch.from_numpy(src).to(dev))
    if q is not None:
        qt = torch.tensor(q, dtype=want.dtype, device=dev)
        negd = torch.from_numpy(neg).to(dev)
        want = torch.where(negd & (want != 0), qt - want, want)
    assert torch.equal(got, want)


def test_closed_form_agrees_with_the_index_map(g):
    """the numpy formula the large-ring checks use is the one the library's index map computes"""
    i = np.arange(1 << 12, dtype=np.int64)
    for poly in (O.X_N_plus, O.X_N_minus):
        for k in (3, 5, 4097, 2 ** 13 - 1):
            for coefficient, dom in ((False, g.DOMAIN_NTT), (True, g.DOMAIN_COEFFICIENT)):
                assert np.array_equal(_closed_form_source(i, k, 12, poly, coefficient),
                                      g.automorphism_index_map(12, k, poly, dom).astype(np.int64))


@pytest.mark.parametrize("logn,batch,ks,poly", [
    (24, 2, [5, 2 ** 25 - 1], O.X_N_plus),
    (24, 3, [3], O.X_N_minus),
    # input 2^29 words, output 9 * 2^29 > 2^32 words (36 GiB): offsets past 2^31 and 2^32 -- an int or unsigned
    # element offset, plane offset g * batch * N or chunk base would wrap, and the top 2^16 words are always checked
    (26, 8, [5, 25, 125, 3, 7, 9, 11, 13, 2 ** 27 - 1], O.X_N_plus),
])
def test_large_rings_ntt_domain_sampled(g, logn, batch, ks, poly):
    import torch
    n = 1 << logn
    d_in = torch.randint(-(1 << 62), 1 << 62, (batch * n,), dtype=torch.int64, device="cuda:0")
    d_out = torch.empty(len(ks) * batch * n, dtype=torch.int64, device="cuda:0")
    g.GPU_Automorphism_NTT(d_in, d_out, ks, logn, poly, batch)
    torch.cuda.synchronize()
    _sampled_check(g, d_in, d_out, ks, logn, poly, batch)
    del d_in, d_out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("logn,batch,ks,poly", [
    (24, 2, [5, 2 ** 25 - 1], O.X_N_plus),
    (26, 1, [7], O.X_N_minus),
    # output 9 * 2^28 > 2^31 words (18 GiB): the gather's offsets past 2^31
    (26, 4, [5, 25, 125, 3, 7, 9, 11, 13, 2 ** 27 - 1], O.X_N_plus),
])
def test_large_rings_coefficient_domain_sampled(g, logn, batch, ks, poly):
    import torch
    q = 576460756061519873
    n = 1 << logn
    d_in = torch.randint(0, q, (batch * n,), dtype=torch.int64, device="cuda:0")
    d_in[:: 1001] = 0
    d_out = torch.empty(len(ks) * batch * n, dtype=torch.int64, device="cuda:0")
    g.GPU_Automorphism(d_in, d_out, ks, g.Modulus(q), logn, poly, batch)
    torch.cuda.synchronize()
    _sampled_check(g, d_in, d_out, ks, logn, poly, batch, q=q)
    del d_in, d_out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("logn", [5, 13, 16])
def test_one_launch_per_call(g, logn):
    import torch
    n, batch = 1 << logn, 3
    d_in = torch.zeros(batch * n, dtype=torch.int64, device="cuda:0")
    for G in (1, 8, 64):
        ks = [(2 * i + 1) % (2 * n) for i in range(G)]
        d_out = torch.empty(G * batch * n, dtype=torch.int64, device="cuda:0")
        with g.launch_log() as log:
            g.GPU_Automorphism_NTT(d_in, d_out, ks, logn, O.X_N_plus, batch)
        assert log.kernels == ["automorphism_ntt"], log.kernels
        with g.launch_log() as log:
            g.GPU_Automorphism(d_in, d_out, ks, g.Modulus(576460756061519873), logn, O.X_N_plus, batch)
        assert len(log.kernels) == 1 and log.kernels[0].startswith("automorphism_coeff"), log.kernels
    torch.cuda.synchronize()


def test_graph_capture_and_replay_with_new_data(g):
    import torch
    logn, poly, batch = 14, O.X_N_plus, 5
    c = MergeCase(g, 64, logn, poly)
    ks = [g.galois_element_for_rotation(1, logn), g.galois_element_for_rotation(-4, logn)]
    d_in = torch.zeros(batch * c.n, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(len(ks) * batch * c.n, dtype=torch.int64, device="cuda:0")
    d_cf = torch.zeros_like(d_out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # eager warm-up on the capture stream
        g.GPU_Automorphism_NTT(d_in, d_out, ks, logn, poly, batch)
        g.GPU_Automorphism(d_in, d_cf, ks, c.prm.modulus, logn, poly, batch)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.GPU_Automorphism_NTT(d_in, d_out, ks, logn, poly, batch)
        g.GPU_Automorphism(d_in, d_cf, ks, c.prm.modulus, logn, poly, batch)
    for seed in (1, 2):
        x = c.random(batch, seed)
        d_in.copy_(g.to_device(x))
        graph.replay()
        torch.cuda.synchronize()
        got = g.to_host(d_out).reshape(len(ks), batch, c.n)
        cf = g.to_host(d_cf).reshape(len(ks), batch, c.n)
        for gi, k in enumerate(ks):
            m = g.automorphism_index_map(logn, k, poly, g.DOMAIN_NTT).astype(np.int64)
            assert np.array_equal(got[gi], x.reshape(batch, c.n)[:, m])
            assert np.array_equal(cf[gi], sigma(x.reshape(batch, c.n), k, poly, c.q))


def test_bad_arguments_are_refused_before_any_launch(g):
    import torch
    logn, batch = 10, 4
    n = 1 << logn
    buf = torch.zeros(4 * batch * n, dtype=torch.int64, device="cuda:0")
    m = g.Modulus(576460756061519873)
    calls = [
        lambda: g.GPU_Automorphism_NTT(buf, buf, [3], logn, O.X_N_plus, batch),            # aliased
        lambda: g.GPU_Automorphism_NTT(buf[: batch * n], buf[n:], [3], logn, O.X_N_plus, batch),  # overlapping
        lambda: g.GPU_Automorphism(buf[n:], buf[:2 * batch * n], [3], m, logn, O.X_N_plus, batch),  # out below in
        lambda: g.GPU_Automorphism_NTT(buf[: batch * n], buf[batch * n:], [4], logn, O.X_N_plus, batch),  # even
        lambda: g.GPU_Automorphism(buf[: batch * n], buf[batch * n:], [3, 2 * n], m, logn, O.X_N_plus, batch),
        lambda: g.GPU_Automorphism_NTT(buf[: batch * n], buf[batch * n:], [], logn, O.X_N_plus, batch),
        lambda: g.GPU_Automorphism_NTT(buf[: batch * n], buf[batch * n:], [3], 29, O.X_N_plus, batch),
        # out holds one plane, two elements need two
        lambda: g.GPU_Automorphism_NTT(buf[: batch * n], buf[batch * n:2 * batch * n], [3, 5], logn, O.X_N_plus, batch),
        lambda: g.GPU_Automorphism(buf[: batch * n - 1], buf[batch * n:], [3], m, logn, O.X_N_plus, batch),  # in short
    ]
    for call in calls:
        with g.launch_log() as log:
            with pytest.raises(ValueError):
                call()
        assert log.kernels == []
    torch.cuda.synchronize()


def test_cpp_caller_of_the_public_header(g):
    """tests/cpp/example_galois.cpp, compiled here against include/ and libgpuntt.so: rotates an NTT-form polynomial with
    GPU_Automorphism_NTT and checks it against NTTCPU of the rotated coefficients"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_galois")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "example_galois.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("13", "3"), ("16", "2", "u32")):
            r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
