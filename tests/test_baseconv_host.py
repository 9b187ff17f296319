"""RNS base conversion without a GPU: the constants a BaseConvPlan uploads (gpuntt_baseconv_constants_*) against Python
integers, and everything the host refuses before a device is touched."""
import math

import pytest

from gpu_utils import find_ntt_factors

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
    ms = moduli(bits, L + K)
    small = min(L, K)
    pick = {ms[i * (L + K) // small] for i in range(small)}
    a, b = [m for m in ms if m in pick], [m for m in ms if m not in pick]
    return (a, b) if L <= K else (b, a)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K", LKS)
def test_constants_against_python_integers(g, bits, L, K):
    qs, ps = bases(bits, L, K)
    c = g.baseconv_constants(qs, ps, bits)
    W, Q = bits, math.prod(qs)
    assert c["matrix"].shape == (L, K)
    for i, q in enumerate(qs):
        qhat = Q // q
        inv = pow(qhat, -1, q)
        b = q.bit_length()
        assert int(c["qhat_inv"][i]) == inv
        assert int(c["qhat_inv_shoup"][i]) == (inv << W) // q
        assert int(c["bit_length"][i]) == b
        R = (1 << (W - 1 + b)) // q
        assert R < (1 << W) and int(c["recip"][i]) == R
        assert [int(v) for v in c["matrix"][i]] == [qhat % p for p in ps]
    assert [int(v) for v in c["q_mod_p"]] == [Q % p for p in ps]
    assert [int(v) for v in c["q_inv_mod_p"]] == [pow(Q, -1, p) for p in ps]


@pytest.mark.parametrize("bits", [64, 32])
def test_recip_is_the_library_s_normalised_reciprocal_formula(g, bits):
    """R_i is what gpuntt_debug_recip_norm_* defines: floor(2^(W-1+b) / q) -- and a power of two, whose R is 2^W, is
    stored as 0 (the kernel shifts instead)"""
    qs = [1 << 20] + moduli(bits, 3)
    c = g.baseconv_constants(qs, [3], bits)
    assert int(c["recip"][0]) == 0 and int(c["bit_length"][0]) == 21
    for i, q in enumerate(qs[1:], 1):
        assert int(c["recip"][i]) == (1 << (bits - 1 + q.bit_length())) // q


def test_non_prime_and_even_moduli_are_accepted(g):
    c = g.baseconv_constants([15015, 1 << 16, 17 * 19], [23 * 29, 31], 64)
    Q = 15015 * (1 << 16) * 17 * 19
    assert [int(v) for v in c["q_mod_p"]] == [Q % (23 * 29), Q % 31]
    assert [int(v) for v in c["q_inv_mod_p"]] == [pow(Q, -1, 23 * 29), pow(Q, -1, 31)]


@pytest.mark.parametrize("bits", [64, 32])
def test_refusals(g, bits):
    ms = moduli(bits, 68)
    refused = [
        ([ms[0], ms[1], ms[0]], [ms[2]]),         # a repeated modulus
        ([15015, 3 * 1009], [ms[2]]),             # input base not pairwise coprime
        ([ms[0], ms[1]], [ms[2], ms[1]]),         # gcd(q_i, p_j) != 1
        ([15015], [ms[0], 13 * 1013]),
        ([], [ms[0]]), ([ms[0]], []),             # counts 0
        (ms[:65], [ms[66]]), ([ms[66]], ms[:65]), # and 65
        ([ms[0], 1], [ms[1]]), ([ms[0]], [0]),    # not a modulus at all
    ]
    for qs, ps in refused:
        with pytest.raises(ValueError):
            g.baseconv_constants(qs, ps, bits)
    for count in (0, 65):
        with pytest.raises(ValueError):
            g.BaseConvPlan.workspace_bytes(count, 4, bits)
        with pytest.raises(ValueError):
            g.BaseConvPlan.workspace_bytes(4, count, bits)
    assert g.BaseConvPlan.workspace_bytes(64, 64, bits) >= (64 * 64 + 3 * 64) * bits // 8
    # a modulus Modulus<T> refuses: its Barrett constant does not fit the word
    bad = (1 << 61) - 1 if bits == 64 else (1 << 30) + 3
    with pytest.raises(ValueError):
        g.baseconv_constants([bad], [ms[0]], bits)
    # ... and one whose three words are not those of its value
    m = g.Modulus(ms[0], bits=bits)
    with pytest.raises(ValueError):
        g.baseconv_constants([g.Modulus(m.value, m.bit, m.mu + 1, bits)], [ms[1]], bits)
    with pytest.raises(ValueError):
        g.baseconv_constants([g.Modulus(ms[0], bits=96 - bits)], [ms[1]], bits)  # the other word width


class _FakeDeviceTensor:
    """what the wrapper's size and type checks look at; the calls below are refused before any pointer is used"""
    is_cuda = True

    def __init__(self, words, itemsize=8, floating=False):
        self._words, self._itemsize = words, itemsize
        self.dtype = type("dtype", (), {"is_floating_point": floating})()

    def numel(self):
        return self._words

    def element_size(self):
        return self._itemsize

    def data_ptr(self):
        raise AssertionError("a refused call must not reach the library")


def test_n_power_and_buffer_checks_need_no_gpu(g):
    """the wrapper refuses short or mistyped buffers and n_power 0 and 29 (the library's own text, "Invalid n_power
    range!") before it asks a tensor for its pointer"""
    import ctypes
    plan = g.BaseConvPlan.__new__(g.BaseConvPlan)  # no device: the wrapper's checks only
    plan.bits, plan.in_count, plan.out_count, plan._h = 64, 3, 5, ctypes.c_void_p()
    n = 1 << 4
    with pytest.raises(ValueError):
        plan._check_buffers(_FakeDeviceTensor(3 * n - 1), (_FakeDeviceTensor(5 * n),), 4, 1)
    with pytest.raises(ValueError):
        plan._check_buffers(_FakeDeviceTensor(3 * n), (_FakeDeviceTensor(5 * n - 1),), 4, 1)
    with pytest.raises(ValueError):
        plan._check_buffers(_FakeDeviceTensor(3 * n, 4), (_FakeDeviceTensor(5 * n),), 4, 1)
    with pytest.raises(ValueError):
        plan._check_buffers(_FakeDeviceTensor(3 * n, 8, True), (_FakeDeviceTensor(5 * n),), 4, 1)
    plan._check_buffers(_FakeDeviceTensor(3 * n), (_FakeDeviceTensor(5 * n),), 4, 1)
    for n_power in (0, 29):
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            plan.convert(_FakeDeviceTensor(1 << 40), _FakeDeviceTensor(1 << 40), n_power, 1)
