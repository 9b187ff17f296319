"""RNS inner product without a GPU (include/gpuntt/rns/inner_product.cuh): the folding constants a plan uploads
(gpuntt_innerprod_constants_*) and the host reference (gpuntt_innerprod_reference_*) against Python integers, and
everything the host refuses before a device is touched.  The reference runs the argument checks of the call itself, so
the refusals are those of multiply_accumulate."""
import ctypes
import itertools

import numpy as np
import pytest

from innerprod_utils import COMPOSITES, WIDTHS, from_words, moduli, operands, ref_inner_product, words


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


@pytest.mark.parametrize("bits", [64, 32])
def test_constants_against_python_integers(g, bits):
    qs = moduli(bits, 12) + [3, 1 << 20]
    assert {q.bit_length() for q in qs} >= set(WIDTHS[bits]) and set(COMPOSITES[bits][:2]) <= set(qs)
    c = g.innerprod_constants(qs, bits)
    W = bits
    for i, q in enumerate(qs):
        t1, t2 = (1 << W) % q, (1 << 2 * W) % q
        assert int(c["pow_w"][i]) == t1 and int(c["pow_w_shoup"][i]) == (t1 << W) // q
        assert int(c["pow_2w"][i]) == t2 and int(c["pow_2w_shoup"][i]) == (t2 << W) // q
        assert int(c["one_shoup"][i]) == (1 << W) // q


def run_reference(g, bits, qs, a, key, out0, n_power, D, count, accumulate, key_mod_count=None, limbs=None):
    C = key.shape[1]
    out = words(g, out0, bits) if accumulate else np.full(out0.size, (1 << bits) - 1, dtype=g.np_dtype(bits))
    wa, wk = words(g, a, bits), words(g, key, bits)
    keep_a, keep_k = wa.copy(), wk.copy()
    got = g.innerprod_reference(qs, wa, wk, out, n_power, D, C, count, accumulate, key_mod_count, limbs, bits)
    assert got is out and np.array_equal(wa, keep_a) and np.array_equal(wk, keep_k)
    return from_words(out, out0.shape)


SHAPES = [(D, C, (1, 3)[i % 2], (1, 3)[(i // 2) % 2])
          for i, (D, C) in enumerate(itertools.product((1, 3, 17, 64), (1, 2, 4)))]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("D,C,count,M", SHAPES)
def test_reference_against_python_integers(g, bits, D, C, count, M):
    """any word value, planted 0, q - 1 and 2^W - 1; the identity and a non-monotone key_limbs into a key with more
    limbs and more digits than the call uses; accumulate off and on"""
    n_power = 3
    qs = moduli(bits, 8)[D % 5:][:M]
    rng = np.random.default_rng(100 * D + 10 * C + count + M + bits)
    perm = {1: [2], 3: [4, 0, 2]}[M]
    for key_mod_count, limbs in ((None, None), (M + 2, None), (M + 2, perm)):
        a, key, out0 = operands(rng, bits, qs, n_power, D, C, count, D + 1, key_mod_count or M)
        for accumulate in (False, True):
            want = ref_inner_product(qs, a, key, out0, D, limbs, accumulate)
            got = run_reference(g, bits, qs, a, key, out0, n_power, D, count, accumulate, key_mod_count, limbs)
            assert np.array_equal(got, want), (key_mod_count, limbs, accumulate)
            assert all((got[:, :, m, :] < q).all() for m, q in enumerate(qs))


@pytest.mark.parametrize("bits", [64, 32])
def test_the_largest_sum_the_contract_allows(g, bits):
    """D = 64, every word of a and of the key 2^W - 1, out prefilled with 2^W - 1, accumulating"""
    qs = moduli(bits, 7)
    top, D, C, count, n_power = (1 << bits) - 1, 64, 2, 1, 1
    M = len(qs)
    a = np.full((D, count, M, 2), top, dtype=object)
    key = np.full((D, C, M, 2), top, dtype=object)
    out0 = np.full((C, count, M, 2), top, dtype=object)
    got = run_reference(g, bits, qs, a, key, out0, n_power, D, count, True)
    for m, q in enumerate(qs):
        assert (got[:, :, m, :] == (top + 64 * top * top) % q).all()
    assert np.array_equal(got, ref_inner_product(qs, a, key, out0, D, None, True))


@pytest.mark.parametrize("bits", [64, 32])
def test_refusals(g, bits):
    dt = g.np_dtype(bits)
    qs = moduli(bits, 3)
    M, n_power, D, C, count = 3, 2, 2, 2, 2
    n = 1 << n_power
    buf = np.zeros((D * count * M + D * C * 5 + C * count * M) * n, dtype=dt)
    a, key, out = np.split(buf, [D * count * M * n, (D * count * M + D * C * 5) * n])

    def call(moduli=qs, a=a, key=key, out=out, n_power=n_power, D=D, C=C, count=count, km=5, limbs=None):
        return g.innerprod_reference(moduli, a, key, out, n_power, D, C, count, False, km, limbs, bits)

    call()
    call(limbs=[4, 0, 4])
    call(count=0)
    refused = [
        dict(D=0), dict(D=65), dict(C=0), dict(C=5), dict(count=-1),        # counts outside their ranges
        dict(km=2), dict(km=257),                                            # key_mod_count below M, above 256
        dict(limbs=[0, 5, 1]), dict(limbs=[0, -1, 1]), dict(limbs=[0, 1]),   # a limb index outside the key, too few
        dict(moduli=[]), dict(moduli=moduli(bits, 65)),                      # 0 and 65 moduli
        dict(moduli=[qs[0], 1, qs[1]]), dict(moduli=[qs[0], 0, qs[1]]),      # not a modulus at all
        dict(a=None), dict(key=None), dict(out=None),                        # null pointers
        dict(out=a), dict(out=buf[n:]), dict(out=key), dict(out=buf[(D * count * M + D * C * 5) * n - 1:]),  # overlaps
        dict(a=a[1:]), dict(key=key[1:]), dict(out=out[1:]),                 # short arrays
        dict(a=a.astype(np.float64)),                                        # not the word type
    ]
    for kw in refused:
        with pytest.raises(ValueError):
            call(**kw)
    # the key's first D digits only: an output right behind them is no overlap even though the key goes on
    call(key=buf[D * count * M * n:], km=5)
    for n_power in (0, 29):
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            call(n_power=n_power)
    with pytest.raises(ValueError, match="null pointer argument"):
        call(key=None)
    # a modulus Modulus<T> refuses: its Barrett constant does not fit the word
    bad = (1 << 61) - 1 if bits == 64 else (1 << 30) + 3
    for fn in (lambda ms: g.innerprod_constants(ms, bits), lambda ms: call(moduli=ms)):
        with pytest.raises(ValueError):
            fn([bad, qs[0], qs[1]])
        # ... one whose three words are not those of its value (the library's existing message) ...
        m = g.Modulus(qs[0], bits=bits)
        with pytest.raises(ValueError, match="Invalid modulus!"):
            fn([g.Modulus(m.value, m.bit, m.mu + 1, bits), qs[1], qs[2]])
        # ... and one of the other word width
        with pytest.raises(ValueError):
            fn([g.Modulus(qs[0], bits=96 - bits), qs[1], qs[2]])
    for ms in ([], moduli(bits, 65)):
        with pytest.raises(ValueError):
            g.innerprod_constants(ms, bits)


@pytest.mark.parametrize("bits", [64, 32])
def test_workspace_bytes(g, bits):
    sizes = [g.InnerProductPlan.workspace_bytes(m, bits) for m in range(1, 65)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s >= 6 * m * bits // 8 for m, s in enumerate(sizes, 1))  # q and the five constants of every modulus
    for m in (0, 65):
        with pytest.raises(ValueError):
            g.InnerProductPlan.workspace_bytes(m, bits)


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
    """the wrapper refuses short or mistyped buffers and n_power 0 and 29 (the library's own text) before it asks a
    tensor for its pointer"""
    plan = g.InnerProductPlan.__new__(g.InnerProductPlan)  # no device: the wrapper's checks only
    plan.bits, plan.mod_count, plan._h = 64, 3, ctypes.c_void_p()
    n_power, D, C, count, km = 4, 2, 2, 3, 5
    n = 1 << n_power
    sizes = [D * count * 3 * n, D * C * km * n, C * count * 3 * n]
    T = _FakeDeviceTensor
    plan._check_buffers(T(sizes[0]), T(sizes[1]), T(sizes[2]), n_power, D, C, count, km)
    for short in range(3):
        bufs = [T(s - (1 if i == short else 0)) for i, s in enumerate(sizes)]
        with pytest.raises(ValueError):
            plan.multiply_accumulate(*bufs, n_power, D, C, count, key_mod_count=km)
    for bad in (T(sizes[0], 4), T(sizes[0], 8, True)):
        with pytest.raises(ValueError):
            plan.multiply_accumulate(bad, T(sizes[1]), T(sizes[2]), n_power, D, C, count, key_mod_count=km)
    with pytest.raises(ValueError):  # the default key_mod_count is M = 3: this key is then long enough, `a` is not
        plan.multiply_accumulate(T(sizes[0] - 1), T(D * C * 3 * n), T(sizes[2]), n_power, D, C, count)
    for bad_power in (0, 29):
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            plan.multiply_accumulate(T(1 << 40), T(1 << 40), T(1 << 40), bad_power, D, C, count)
