"""The samplers of include/gpuntt/rns/sampling.cuh without a GPU: the Philox known answers through the C ABI, the host
references against tests/sampling_exact.py word for word, the rejection and tail paths, and the distributions on the
model with bounds derived from the distributions themselves."""
import ctypes
import math

import numpy as np
import pytest

import sampling_exact as SE


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


# Random123's known answers for philox4x32_10
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

# just above a power of two (half the candidates reject), just below one (none should), a small composite, and 1
MODULI = {64: [2**60 + 33, 2**61 - 1, 15015, 1, 2**62 + 135], 32: [2**30 + 3, 2**31 - 1, 15015, 1, 2**28 + 1]}
ABOVE = {64: 2**60 + 33, 32: 2**30 + 3}
BELOW = {64: 2**61 - 1, 32: 2**31 - 1}


def test_philox_known_answers(g):
    for ctr, key, want in KAT:
        assert tuple(g.philox4x32_10(ctr, key)) == want
        assert tuple(SE.philox(ctr, key)) == want


def test_entry_points_refuse_without_a_device(g):
    lib = g.load_library()
    word = (ctypes.c_uint64 * 4)(1, 1, 1, 1)
    p = ctypes.cast(word, ctypes.c_void_p)
    assert lib.gpuntt_philox4x32_10(None, p, p) != 0
    assert lib.gpuntt_sample_small(None, 1, 4, 0, ctypes.c_uint64(1), 0, None) != 0
    assert lib.gpuntt_sample_reference_small(p, 1, 4, 2, ctypes.c_uint64(1), 0) != 0  # no such distribution
    for s in ("u32", "u64"):
        uni = getattr(lib, "gpuntt_sample_uniform_" + s)
        ref = getattr(lib, "gpuntt_sample_reference_uniform_" + s)
        assert uni(None, p, 1, 4, 1, ctypes.c_uint64(16), ctypes.c_uint64(1), 0, None) != 0
        assert ref(p, p, 0, 1, 1, ctypes.c_uint64(2), ctypes.c_uint64(1), 0, 32) != 0   # mod_count
        assert ref(p, p, 1, 1, 1, ctypes.c_uint64(1), ctypes.c_uint64(1), 0, 32) != 0   # stride below mod_count * N
        assert ref(p, p, 1, 1, 1, ctypes.c_uint64(2), ctypes.c_uint64(1), 0, 0) != 0    # max_candidates
        lift = getattr(lib, "gpuntt_keyswitch_plan_lift_small_" + s)
        gen = getattr(lib, "gpuntt_keyswitch_plan_generate_keys_" + s)
        enc = getattr(lib, "gpuntt_keyswitch_plan_encrypt_symmetric_" + s)
        assert lift(None, p, p, 1, 1, 0, None) != 0
        assert gen(None, p, p, p, p, 1, p, None) != 0
        assert enc(None, p, p, p, p, 1, p, None) != 0
    with pytest.raises(ValueError):
        g.sample_reference_uniform([0], 2, 1, seed=1)  # a modulus 0


@pytest.mark.parametrize("bits", [64, 32])
def test_uniform_reference_equals_the_model_word_for_word(g, bits):
    qs, n_power, stacks, seed, sid = MODULI[bits], 5, 3, 0x0123456789ABCDEF, 7
    want, used = SE.exact_uniform(qs, n_power, stacks, bits, seed, sid)
    got = g.sample_reference_uniform(qs, n_power, stacks, seed, sid, bits=bits)
    assert np.array_equal(got.astype(object).reshape(want.shape), want)
    for m, q in enumerate(qs):
        assert (want[:, m, :] < q).all()
    # strided stacks: the words do not move (the index is dense) and the gaps are not written
    stride = (len(qs) << n_power) + 24
    got = g.sample_reference_uniform(qs, n_power, stacks, seed, sid, stack_stride_words=stride, bits=bits, fill=0x5A)
    dense = len(qs) << n_power
    for s in range(stacks):
        assert np.array_equal(got[s * stride:s * stride + dense].astype(object), want[s].reshape(-1))
        assert (got[s * stride + dense:(s + 1) * stride] == 0x5A).all()
    # another stream, another seed: other words
    assert not np.array_equal(g.sample_reference_uniform(qs, n_power, 1, seed, sid + 1, bits=bits)[:64],
                              g.sample_reference_uniform(qs, n_power, 1, seed, sid, bits=bits)[:64])
    assert not np.array_equal(g.sample_reference_uniform(qs, n_power, 1, seed + 1, sid, bits=bits)[:64],
                              g.sample_reference_uniform(qs, n_power, 1, seed, sid, bits=bits)[:64])


@pytest.mark.parametrize("bits", [64, 32])
def test_rejection_path(g, bits):
    """a modulus just above a power of two rejects about half of its candidates, one just below rejects none; both
    through the k-candidates-per-block layout, and the reference follows the model through them"""
    n_power = 12
    qs = [ABOVE[bits], BELOW[bits]]
    want, used = SE.exact_uniform(qs, n_power, 1, bits, seed=99, stream_id=3)
    second = (used[0, 0] >= 2).mean()
    print("fraction of words that need a second candidate: %.3f (%d bits)" % (second, bits))
    assert second >= 0.25
    assert used[0, 0].max() > (2 if bits == 64 else 4)  # a word that went on into the second Philox block
    # 2^b - 1: only the candidate 2^b - 1 itself is rejected, probability 2^-61 / 2^-31 per candidate
    assert (used[0, 1] == 1).all()
    got = g.sample_reference_uniform(qs, n_power, 1, 99, 3, bits=bits)
    assert np.array_equal(got.astype(object).reshape(want.shape), want)


@pytest.mark.parametrize("bits", [64, 32])
def test_tail_path(g, bits):
    """max_candidates = 1: every rejected word is the candidate's r mod q"""
    qs, n_power = [ABOVE[bits], 15015, 3], 8
    want, used = SE.exact_uniform(qs, n_power, 2, bits, seed=5, stream_id=0, max_candidates=1)
    full, _ = SE.exact_uniform(qs, n_power, 2, bits, seed=5, stream_id=0)
    assert (want != full).sum() > 100  # the tail was taken, and it is not what the full loop returns
    got = g.sample_reference_uniform(qs, n_power, 2, 5, 0, bits=bits, max_candidates=1)
    assert np.array_equal(got.astype(object).reshape(want.shape), want)
    for m, q in enumerate(qs):
        assert (want[:, m, :] < q).all()
    # 3 candidates: the loop stops inside a Philox block
    want3, _ = SE.exact_uniform(qs, n_power, 1, bits, seed=5, stream_id=0, max_candidates=3)
    got3 = g.sample_reference_uniform(qs, n_power, 1, 5, 0, bits=bits, max_candidates=3)
    assert np.array_equal(got3.astype(object).reshape(want3.shape), want3)


@pytest.mark.parametrize("distribution", [SE.TERNARY, SE.CBD21])
def test_small_reference_equals_the_model(g, distribution):
    want = SE.exact_small(3, 6, distribution, seed=0xFEEDFACE12345678, stream_id=9)
    got = g.sample_reference_small(3, 6, distribution, 0xFEEDFACE12345678, 9)
    assert np.array_equal(got.reshape(want.shape), want)


def test_ternary_scan_skips_fields_of_three():
    """the scan itself, on blocks built by hand: the model and the reference share only the definition"""
    def scan(x):
        for f in range(64):
            v = (x >> (2 * f)) & 3
            if v != 3:
                return v - 1
        return 0
    assert scan((1 << 128) - 1) == 0
    assert scan(((1 << 128) - 1) ^ (1 << 127)) == 0       # the last field is 1: value 0
    assert scan(((1 << 128) - 1) ^ (3 << 66)) == -1       # field 33 (word 2) is 0
    assert scan(0b1011) == 1                              # field 0 is 3, field 1 is 2


def test_distributions_on_the_model():
    """n = 2^16 words.  Ternary: each count is Binomial(n, 1/3), standard deviation sqrt(2 n / 9): six of them.  CBD21:
    variance 10.5, so the mean of n values has standard deviation sqrt(10.5 / n): six of them; |v| <= 21 always."""
    n_power = 16
    n = 1 << n_power
    t = SE.exact_small(1, n_power, SE.TERNARY, seed=2024, stream_id=1).reshape(-1)
    assert set(np.unique(t)) == {-1, 0, 1}
    for v in (-1, 0, 1):
        assert abs(int((t == v).sum()) - n / 3) <= 6 * math.sqrt(2 * n / 9), v
    c = SE.exact_small(1, n_power, SE.CBD21, seed=2024, stream_id=2).reshape(-1).astype(np.int64)
    assert abs(c.mean()) <= 6 * math.sqrt(10.5 / n)
    assert np.abs(c).max() <= 21
    assert 9.5 < c.var() < 11.5  # the variance of n samples of a bounded variable: far inside


def test_reference_distributions(g):
    """the same bounds on the reference at 2^16 (it is fast), so a reference that followed a wrong model would show"""
    n = 1 << 16
    t = g.sample_reference_small(1, 16, g.TERNARY, 77, 0)
    for v in (-1, 0, 1):
        assert abs(int((t == v).sum()) - n / 3) <= 6 * math.sqrt(2 * n / 9), v
    c = g.sample_reference_small(1, 16, g.CBD21, 77, 0).astype(np.int64)
    assert abs(c.mean()) <= 6 * math.sqrt(10.5 / n) and np.abs(c).max() <= 21
    for bits in (64, 32):
        q = ABOVE[bits]
        u = g.sample_reference_uniform([q], 16, 1, 77, 0, bits=bits)
        assert (u < q).all()
        # uniform on [0, q): the mean of n values has standard deviation q / sqrt(12 n)
        assert abs(float(u.astype(np.float64).mean()) - q / 2) <= 6 * q / math.sqrt(12 * n)
