"""CPU-side tests of the Galois automorphisms (include/gpuntt/ntt_merge/galois.cuh): the index maps the kernels use,
read back through gpuntt_automorphism_index_map, against the oracle's NTTCPU and numpy sigma_k; the Galois element
helpers; the argument checks.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O


@pytest.fixture(scope="module")
def g(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    pkg.load_library()
    return pkg


def sigma(x, k, poly, q):
    """sigma_k(a)(X) = a(X^k) in Z_q[X]/(X^N + 1) (X_N_plus) or Z_q[X]/(X^N - 1), numpy, one polynomial or a batch"""
    x = np.asarray(x, dtype=np.uint64)
    n = x.shape[-1]
    j = np.arange(n, dtype=np.int64)
    if poly == O.X_N_plus:
        e = (k * j) % (2 * n)
        neg = e >= n
        vals = np.where(neg, (np.uint64(q) - x) % np.uint64(q), x)
        out = np.empty_like(x)
        out[..., e % n] = vals
        return out
    out = np.empty_like(x)
    out[..., (k * j) % n] = x
    return out


def elements(logn):
    two_n = 2 << logn
    ks = {1, 3 % two_n, 5 % two_n, two_n - 1}
    ks |= {pow(5, r, two_n) for r in (2, 7, -1, -3)}
    return sorted(k for k in ks if k % 2)


def oracle_map(P, logn, poly, k, seed):
    """the NTT-domain map derived from the oracle alone: NTT(sigma_k(x))[i] == NTT(x)[map[i]]"""
    prm = P.merge_params(logn, poly)
    q = prm["mod"][0]
    x = P.splitmix(seed, 0, 1 << logn, q)
    y = P.merge_ntt(x, prm)
    z = P.merge_ntt(sigma(x, k, poly, q), prm)
    order = np.argsort(y, kind="stable")
    assert np.unique(y).size == y.size  # 64-bit prime: collisions are negligible, but a collision would fool the match
    idx = order[np.searchsorted(y[order], z)]
    assert np.array_equal(y[idx], z)
    return idx.astype(np.uint32)


@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", list(range(1, 15)))
def test_ntt_domain_map_matches_oracle(g, logn, poly):
    P = O.Port(64)
    for k in elements(logn):  # X_N_minus reduces the elements mod N
        got = g.automorphism_index_map(logn, k, poly, g.DOMAIN_NTT)
        assert np.array_equal(got, oracle_map(P, logn, poly, k, seed=1000 * logn + k)), (logn, poly, k)


@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", [1, 2, 3, 6, 11, 14])
def test_coefficient_map_matches_numpy_sigma(g, logn, poly):
    n, q = 1 << logn, 576460756061519873
    rng = np.random.default_rng(logn)
    x = rng.integers(0, q, size=n, dtype=np.uint64)
    x[0] = 0  # the negation maps 0 to 0, not to q
    for k in elements(logn):
        m = g.automorphism_index_map(logn, k, poly, g.DOMAIN_COEFFICIENT).astype(np.int64)
        if poly == O.X_N_plus:
            assert m.max() < 2 * n
            got = np.where(m < n, x[m % n], (np.uint64(q) - x[m % n]) % np.uint64(q))
        else:
            assert m.max() < n
            got = x[m]
        assert np.array_equal(got, sigma(x, k, poly, q)), (logn, poly, k)


@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", [1, 2, 4, 9, 13, 16])
def test_maps_are_bijections_with_the_chunk_property(g, logn, poly):
    """every output chunk of 2^(n-s) consecutive slots reads exactly one input chunk of the same size, for every s: the
    property the NTT-domain kernel's one-chunk-per-workgroup design rests on"""
    n = 1 << logn
    i = np.arange(n, dtype=np.uint32)
    for k in elements(logn):
        m = g.automorphism_index_map(logn, k, poly, g.DOMAIN_NTT)
        assert np.array_equal(np.sort(m), i)
        for s in range(logn + 1):
            pairs = np.unique((i >> (logn - s)).astype(np.uint64) << 32 | (m >> (logn - s)).astype(np.uint64))
            assert pairs.size == 1 << s, (k, s)
        c = g.automorphism_index_map(logn, k, poly, g.DOMAIN_COEFFICIENT)
        assert np.array_equal(np.sort(c % n), i)


@pytest.mark.parametrize("poly", [O.X_N_plus, O.X_N_minus])
@pytest.mark.parametrize("logn", [3, 8, 12])
def test_maps_compose(g, logn, poly):
    """sigma_k o sigma_l = sigma_kl: applying l's map after k's equals kl's map, in both domains"""
    n, q = 1 << logn, 12289 if logn <= 10 else 576460756061519873
    mod = (2 * n) if poly == O.X_N_plus else n
    x = np.random.default_rng(5).integers(0, q, size=n, dtype=np.uint64)
    ks = elements(logn)
    for k in ks:
        for l in ks:
            mk = g.automorphism_index_map(logn, k, poly, g.DOMAIN_NTT)
            ml = g.automorphism_index_map(logn, l, poly, g.DOMAIN_NTT)
            mkl = g.automorphism_index_map(logn, (k * l) % mod, poly, g.DOMAIN_NTT)
            assert np.array_equal(ml[mk], mkl)
            assert np.array_equal(sigma(sigma(x, l, poly, q), k, poly, q), sigma(x, (k * l) % mod, poly, q))


def test_galois_elements(g):
    for logn in (1, 2, 3, 10, 16, 28):
        two_n = 2 << logn
        for r in (0, 1, 2, 3, 7, 100, -1, -2, -7, -100, (1 << logn) // 2, 12345):
            assert g.galois_element_for_rotation(r, logn) == pow(5, r, two_n), (logn, r)
        assert g.galois_element_for_conjugation(logn) == two_n - 1
    with pytest.raises(ValueError, match="Invalid n_power range!"):
        g.galois_element_for_rotation(1, 29)
    with pytest.raises(ValueError, match="Invalid n_power range!"):
        g.galois_element_for_conjugation(0)


def test_invalid_arguments_are_refused(g):
    """even / zero elements, a count outside [1, 64], n_power outside [1, 28]: GPUNTT_ERR_INVALID_ARGUMENT.  The data
    calls get batch_size 0, so nothing could be launched even if a check were missing."""
    lib = g.load_library()
    ERR = -1
    fake_in, fake_out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    m64 = g._M64(576460756061519873, 60, 0)

    def elts(*ks):
        return (ctypes.c_uint32 * max(1, len(ks)))(*ks)

    buf = np.empty(1 << 10, dtype=np.uint32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(4), 0, 0, p) == ERR
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(0), 1, 1, p) == ERR
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(2048), 0, 0, p) == ERR  # 2N = 0 mod 2N: even
    assert lib.gpuntt_automorphism_index_map(0, ctypes.c_uint32(3), 0, 0, p) == ERR
    assert lib.gpuntt_automorphism_index_map(29, ctypes.c_uint32(3), 0, 0, p) == ERR
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(3), 2, 0, p) == ERR
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(3), 0, 2, p) == ERR
    assert lib.gpuntt_automorphism_index_map(10, ctypes.c_uint32(3), 0, 0, p) == 0
    for bits in (32, 64):
        f = getattr(lib, "gpuntt_automorphism_ntt_u%d" % bits)
        assert f(fake_in, fake_out, elts(4), 1, 10, 0, None, 0) == ERR
        assert f(fake_in, fake_out, elts(3, 0), 2, 10, 0, None, 0) == ERR
        assert f(fake_in, fake_out, elts(), 0, 10, 0, None, 0) == ERR
        assert f(fake_in, fake_out, elts(*([3] * 65)), 65, 10, 0, None, 0) == ERR
        assert f(fake_in, fake_out, elts(3), 1, 0, 0, None, 0) == ERR
        assert f(fake_in, fake_out, elts(3), 1, 29, 0, None, 0) == ERR
        assert "Invalid n_power range!" in lib.gpuntt_last_error().decode()
        assert f(fake_in, fake_in, elts(3), 1, 10, 0, None, 0) == ERR  # same buffer
    assert lib.gpuntt_automorphism_u64(fake_in, fake_out, elts(6), 1, m64, 10, 0, None, 0) == ERR
    assert lib.gpuntt_automorphism_u64(fake_in, fake_out, elts(), 0, m64, 10, 0, None, 0) == ERR
    assert lib.gpuntt_automorphism_rns_u64(fake_in, fake_out, elts(3), 1, fake_in, 10, 0, None, 0, 0) == ERR
    assert lib.gpuntt_automorphism_rns_u64(fake_in, fake_out, elts(8), 1, fake_in, 10, 0, None, 0, 1) == ERR
    with pytest.raises(ValueError):
        g.automorphism_index_map(10, 6, O.X_N_plus)
    for n_power in (0, 29, 40):  # refused before the N-entry host array is allocated
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            g.automorphism_index_map(n_power, 3, O.X_N_plus)
