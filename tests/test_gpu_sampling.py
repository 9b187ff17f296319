"""sample_uniform / sample_small (include/gpuntt/rns/sampling.cuh) on the GPU: every word against tests/sampling_exact.py
for both word widths at n_power 1, 3 and 12 -- dense, one word off alignment (the one-word stores) and strided as the `a`
planes of a switching key, with the words between and behind the stacks untouched --, the same words from two launches,
other words from another stream, and the refusals, before any launch."""
import numpy as np
import pytest

import sampling_exact as SE
from hoisted_utils import filled

pytestmark = pytest.mark.gpu

# just above a power of two (the rejection path), just below one, a small composite
MODULI = {64: [2**60 + 33, 2**61 - 1, 15015], 32: [2**30 + 3, 2**31 - 1, 15015]}
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module")
def model():
    """the model's words, computed once per (bits, n_power): [2 stacks][3 moduli][N]"""
    cache = {}

    def get(bits, n_power):
        if (bits, n_power) not in cache:
            cache[(bits, n_power)] = SE.exact_uniform(MODULI[bits], n_power, 2, bits, seed=0xC0FFEE0123456789,
                                                      stream_id=5)[0]
        return cache[(bits, n_power)]
    return get


def host(g, t, shape):
    return g.to_host(t).astype(object).reshape(shape)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 3, 12])
def test_uniform_every_word_dense_and_off_alignment(g, model, bits, n_power):
    import torch
    qs, n = MODULI[bits], 1 << n_power
    want = model(bits, n_power)
    words = 2 * len(qs) * n
    for offset in (0, 1):
        buf = filled(bits, words + 32, offset, GUARD)
        with g.launch_log() as log:
            g.sample_uniform(buf, qs, n_power, 2, 0xC0FFEE0123456789, 5)
        torch.cuda.synchronize()
        assert log.kernels == ["sample_uniform_words"], log.kernels
        assert np.array_equal(host(g, buf[:words], want.shape), want), offset
        assert (g.to_host(buf[words:]) == GUARD).all(), offset


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 3, 12])
def test_uniform_fills_the_a_planes_of_a_key_in_place(g, model, bits, n_power):
    """key T[D = 2][2][M = 3][N]: out = key + M N, stacks = D, stride 2 M N; component 0 and the words behind the key
    keep their guard value, and the words are those of the dense call (the index is dense)"""
    import torch
    qs, n = MODULI[bits], 1 << n_power
    M, D = len(qs), 2
    want = model(bits, n_power)
    key = filled(bits, D * 2 * M * n + 32, 0, GUARD)
    g.sample_uniform(key[M * n:D * 2 * M * n], qs, n_power, D, 0xC0FFEE0123456789, 5, stack_stride_words=2 * M * n)
    torch.cuda.synchronize()
    got = host(g, key[:D * 2 * M * n], (D, 2, M, n))
    assert np.array_equal(got[:, 1], want)
    assert (got[:, 0] == GUARD).all()
    assert (g.to_host(key[D * 2 * M * n:]) == GUARD).all()
    # a stride that is no multiple of 16 bytes: the one-word stores
    odd = 2 * M * n + 1
    buf = filled(bits, odd + M * n + 32, 0, GUARD)
    g.sample_uniform(buf[:odd + M * n], qs, n_power, D, 0xC0FFEE0123456789, 5, stack_stride_words=odd)
    torch.cuda.synchronize()
    flat = g.to_host(buf).astype(object)
    assert np.array_equal(flat[:M * n].reshape(M, n), want[0]) and np.array_equal(flat[odd:odd + M * n].reshape(M, n), want[1])
    assert (flat[M * n:odd] == GUARD).all() and (flat[odd + M * n:] == GUARD).all()


@pytest.mark.parametrize("bits", [64, 32])
def test_uniform_equals_the_host_reference_and_is_reproducible(g, bits):
    """n_power 12, six moduli, three stacks against the library's own host reference (the model is checked against it
    without a GPU); two launches give the same words, another stream or seed gives others"""
    import torch
    qs = MODULI[bits] + [3, 1, (1 << (bits - 1)) + 1]
    n_power, stacks = 12, 3
    words = stacks * len(qs) << n_power
    a, b, c, d = (filled(bits, words, 0, GUARD) for _ in range(4))
    g.sample_uniform(a, qs, n_power, stacks, 11, 2)
    g.sample_uniform(b, qs, n_power, stacks, 11, 2)
    g.sample_uniform(c, qs, n_power, stacks, 11, 3)
    g.sample_uniform(d, qs, n_power, stacks, 12, 2)
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(a), g.sample_reference_uniform(qs, n_power, stacks, 11, 2, bits=bits))
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and not torch.equal(a, d)
    got = host(g, a, (stacks, len(qs), 1 << n_power))
    for m, q in enumerate(qs):
        assert (got[:, m, :] < q).all()


@pytest.mark.parametrize("distribution", [SE.TERNARY, SE.CBD21])
@pytest.mark.parametrize("n_power", [1, 3, 12])
def test_small_every_word(g, distribution, n_power):
    import torch
    polys, n = 3, 1 << n_power
    want = SE.exact_small(polys, n_power, distribution, seed=0xABCDEF9876543210, stream_id=8)
    for offset in (0, 1):
        buf = filled(32, polys * n + 32, offset, GUARD)
        with g.launch_log() as log:
            g.sample_small(buf, polys, n_power, distribution, 0xABCDEF9876543210, 8)
        torch.cuda.synchronize()
        assert log.kernels == ["sample_small_words"], log.kernels
        assert np.array_equal(g.to_host(buf[:polys * n], signed=True).reshape(polys, n), want), offset
        assert (g.to_host(buf[polys * n:]) == GUARD).all(), offset
    other = filled(32, polys * n, 0, GUARD)
    g.sample_small(other, polys, n_power, distribution, 0xABCDEF9876543210, 9)
    torch.cuda.synchronize()
    assert not np.array_equal(g.to_host(other, signed=True).reshape(polys, n), want) or n_power == 1


def test_nothing_to_do_and_refusals(g):
    import torch
    qs, n_power = MODULI[64], 3
    n = 1 << n_power
    buf = filled(64, 2 * len(qs) * n, 0, GUARD)
    small = filled(32, 2 * n, 0, GUARD)
    with g.launch_log() as log:
        g.sample_uniform(buf, qs, n_power, 0, 1)
        g.sample_small(small, 0, n_power, g.TERNARY, 1)
    assert log.kernels == []
    lib = g.load_library()
    import ctypes
    p = ctypes.c_void_p(buf.data_ptr())
    arr = (ctypes.c_uint64 * 3)(*qs)
    zero = (ctypes.c_uint64 * 3)(qs[0], 0, qs[2])
    u64 = ctypes.c_uint64
    raw = lib.gpuntt_sample_uniform_u64
    refused = [lambda: g.sample_uniform(None, qs, n_power, 2, 1),
               lambda: g.sample_uniform(buf, qs, n_power, 3, 1),                       # too small
               lambda: g.sample_uniform(buf, qs, n_power, 2, 1, stack_stride_words=len(qs) * n - 1),
               lambda: g.sample_uniform(buf, [], n_power, 2, 1),
               lambda: g.sample_uniform(buf, [3] * 257, 1, 1, 1),
               lambda: g.sample_uniform(buf, [qs[0], 0], n_power, 2, 1),
               lambda: g.sample_uniform(buf, qs, 0, 2, 1),
               lambda: g.sample_uniform(buf, qs, 29, 0, 1),
               lambda: g.sample_uniform(buf, qs, n_power, -1, 1),
               lambda: g.sample_uniform(buf.to(torch.float64), qs, n_power, 2, 1),
               lambda: g.sample_small(None, 2, n_power, g.TERNARY, 1),
               lambda: g.sample_small(small, 3, n_power, g.TERNARY, 1),                # too small
               lambda: g.sample_small(small, 2, n_power, 2, 1),                        # no such distribution
               lambda: g.sample_small(small, -1, n_power, g.CBD21, 1),
               lambda: g.sample_small(small, 2, 0, g.CBD21, 1),
               lambda: g.sample_small(buf, 2, n_power, g.CBD21, 1),                    # not a 32-bit tensor
               # the library's own checks, past the wrapper
               lambda: g._check(raw(p, zero, 3, n_power, 2, u64(3 * n), u64(1), 0, None)),
               lambda: g._check(raw(p, arr, 3, n_power, 2, u64(3 * n - 1), u64(1), 0, None)),
               lambda: g._check(raw(p, arr, 257, n_power, 2, u64(257 * n), u64(1), 0, None)),
               lambda: g._check(raw(p, arr, 3, n_power, -1, u64(3 * n), u64(1), 0, None)),
               lambda: g._check(raw(None, arr, 3, n_power, 2, u64(3 * n), u64(1), 0, None))]
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises((ValueError, RuntimeError)):
                f()
        assert log.kernels == [], i
    torch.cuda.synchronize()
    assert (g.to_host(buf) == GUARD).all() and (g.to_host(small) == GUARD).all()
