"""KeySwitchPlan.rotate_hoisted and rotate_hoisted_sum on the MI355X against the exact-integer reference of
tests/hoisted_exact.py: no GPU call on the expected side, array_equal on every output word.  Rings of the widest primes
Modulus<T> accepts -- 62/61/62/60 and 30/29/30/28 bits, found from the top ("wide"), and 62- / 30-bit primes spread over
the eighth below 2^(W-2) ("spread": see hoisted_utils.spread_factors for why the top alone does not reach the edge) --
and one ring of 45- / 20-bit primes for contrast; operands of arbitrary words with 0, 2^W - 1, q - 1 and q planted; the
shapes at which the kernels change behaviour; the largest sums the contract allows."""
import itertools

import numpy as np
import pytest

from hoisted_exact import NARROW, exact_u, exact_weighted_sum, finish
from hoisted_sum_utils import with_nones
from hoisted_utils import any_words, device_words, elements_for, filled, make_plan, ring
from innerprod_utils import from_words, words

pytestmark = pytest.mark.gpu

KERNELS = ["rotate", "sum"]


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


@pytest.fixture
def chunk6(g):
    g.set_test_hook("keyswitch_hoist_chunk", 6)
    yield
    g.set_test_hook("keyswitch_hoist_chunk", 0)


def the_ring(g, bits, n_power, M, kind, poly=None):
    return ring(g, bits, n_power, M=M, poly=poly, widths=NARROW[bits] if kind == "narrow" else kind)


class Case:
    """one plan with its operands on the host (numpy words, and as Python integers) and on the device"""

    def __init__(self, g, full, limbs, L, alpha, bits, rng, G, count, offset=0, host=None, **plan_kw):
        self.g, self.bits, self.L, self.G, self.count, self.offset = g, bits, L, G, count, offset
        self.st = full.sub(limbs)
        self.cases = [full.cases[i] for i in limbs]
        self.qs, self.n_power, self.n = self.st["moduli"], full.n_power, full.n
        self.plan = make_plan(g, self.st, L, alpha, full.n_power, bits, **plan_kw)
        self.key_limbs = plan_kw.get("key_limbs")
        self.M, self.D, self.KM = len(limbs), self.plan.digits, plan_kw.get("key_mod_count", len(limbs))
        self.elts = elements_for(g, full.n_power, G)
        M, D, KM, n = self.M, self.D, self.KM, self.n
        if host is None:
            host = dict(a=any_words(g, rng, bits, D * count * M * n, self.qs),
                        c0=any_words(g, rng, bits, count * L * n, self.qs[:L]),
                        keys=[any_words(g, rng, bits, D * 2 * KM * n, full.moduli) for _ in range(G)],
                        weights=[any_words(g, rng, bits, M * n, self.qs) for _ in range(G)])
        else:
            host = host(self)
        self.a, self.c0 = device_words(g, host["a"], offset), device_words(g, host["c0"], offset)
        self.keys = [device_words(g, k, offset) for k in host["keys"]]
        self.weights = [device_words(g, w, offset) for w in host["weights"]]
        self.keep = [t.clone() for t in (self.a, self.c0, *self.keys, *self.weights)]
        a, c0 = from_words(host["a"], (D, count, M, n)), from_words(host["c0"], (count, L, n))
        keys = [from_words(k, (D, 2, KM, n)) for k in host["keys"]]
        self.w_int = [from_words(w, (M, n)) for w in host["weights"]]
        poly = self.st["poly"]
        self.u = {with_c0: exact_u(g, self.qs, L, self.n_power, poly, a, c0 if with_c0 else None, keys, self.elts,
                                   self.key_limbs) for with_c0 in (False, True)}

    def weight_list(self, which):
        """which: None -- no list; "all" -- every weight; an int -- a None at that entry and every fourth after it
        (hoisted_sum_utils.with_nones).  Returns the device list and the integer list"""
        if which is None:
            return None, None
        if which == "all":
            return self.weights, self.w_int
        return with_nones(self.weights, which), with_nones(self.w_int, which)

    def run(self, kernel, with_c0, output_ntt, which=None, out=None, scratch=None):
        """one call on the GPU and the exact expected words, both flat numpy arrays"""
        import torch
        g, plan, bits, G, count = self.g, self.plan, self.bits, self.G, self.count
        c0 = self.c0 if with_c0 else None
        if kernel == "rotate":
            want = finish(self.cases, self.L, self.u[with_c0], bits, output_ntt)
            out = filled(bits, want.size, self.offset) if out is None else out
            if scratch is None:
                scratch = torch.zeros(plan.hoisted_scratch_bytes(count, G), dtype=torch.uint8, device="cuda:0")
            plan.rotate_hoisted(self.a, c0, self.keys, self.elts, out, count, output_ntt, scratch)
        else:
            d_w, w = self.weight_list(which)
            want = finish(self.cases, self.L, exact_weighted_sum(self.qs, self.u[with_c0], w), bits, output_ntt)
            out = filled(bits, want.size, self.offset) if out is None else out
            if scratch is None:
                scratch = torch.zeros(plan.hoisted_sum_scratch_bytes(count), dtype=torch.uint8, device="cuda:0")
            plan.rotate_hoisted_sum(self.a, c0, self.keys, self.elts, d_w, out, count, output_ntt, scratch)
        torch.cuda.synchronize()
        return g.to_host(out), words(g, want, bits)

    def check(self, kernel, combos=None):
        """c0 present / absent x output_ntt on / off; for the sum the weights None once, otherwise with None entries"""
        import torch
        which = {(False, False): None, (False, True): 0, (True, False): 1, (True, True): 2 if self.G > 2 else 1}
        for with_c0, output_ntt in combos or itertools.product((False, True), (False, True)):
            got, want = self.run(kernel, with_c0, output_ntt, which[(with_c0, output_ntt)])
            assert np.array_equal(got, want), (kernel, self.G, self.count, with_c0, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip((self.a, self.c0, *self.keys, *self.weights), self.keep)), \
            "an input was modified"


def whole(g, bits, n_power, L, K, alpha, kind, rng, G, count, poly=None, **kw):
    M = L + K
    return Case(g, the_ring(g, bits, n_power, max(M, 8), kind, poly), list(range(M)), L, alpha, bits, rng, G, count, **kw)


COMBOS = [(5, 3), (1, 1)]
# the widest primes at every ring; the spread ones where a chunk is full: one chunk exactly and two chunks
RINGS_AND_SIZES = [("wide", 5), ("wide", 6), ("wide", 7), ("wide", 9), ("spread", 6), ("spread", 7)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kind,n_power", RINGS_AND_SIZES)
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_output_word_with_chunks_of_64_slots(g, chunk6, kernel, L, K, alpha, kind, n_power, bits):
    """n_power 5: below a chunk, lanes without a slot; 6: one chunk exactly; 7: two chunks, the destination differs from
    the source; 9: eight"""
    rng = np.random.default_rng(1000 * n_power + 10 * L + bits)
    for G, count in COMBOS:
        whole(g, bits, n_power, L, K, alpha, kind, rng, G, count).check(kernel)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_narrow_ring(g, chunk6, kernel, bits):
    """primes of 45 / 20 bits: far from every edge of the word, the same words expected"""
    whole(g, bits, 7, 3, 2, 2, "narrow", np.random.default_rng(45 + bits), 5, 3).check(kernel)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_automatic_chunk(g, kernel, bits):
    n_power = 9
    c = whole(g, bits, n_power, 6, 2, 2, "wide", np.random.default_rng(9 + bits), 5, 3)
    chunk = g.keyswitch_hoist_chunk if kernel == "rotate" else g.keyswitch_hoist_sum_chunk
    assert chunk(bits, c.D, n_power) > 6
    c.check(kernel)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_cyclic_ring(g, kernel, bits):
    """a plan built with X_N_minus: elements reduced mod N, the cyclic slot order"""
    whole(g, bits, 7, 3, 2, 2, "wide", np.random.default_rng(7 + bits), 5, 3, poly=g.X_N_minus).check(kernel)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_lower_level_plan_reads_the_full_level_keys_in_place(g, kernel, bits):
    """L = 4 of keys built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    limbs = [0, 1, 2, 3, 6, 7]
    full = the_ring(g, bits, 7, 8, "spread")
    Case(g, full, limbs, 4, 2, bits, np.random.default_rng(bits), 5, 3, key_mod_count=8, key_limbs=limbs).check(kernel)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_base_pointers_one_word_off_alignment(g, kernel, bits):
    """a, c0, the keys, the weights and out one word off 16-byte alignment: the loaders' one-word path"""
    c = whole(g, bits, 7, 3, 2, 2, "spread", np.random.default_rng(1 + bits), 5, 3, offset=1)
    assert c.a.data_ptr() % 16 and c.c0.data_ptr() % 16 and c.keys[0].data_ptr() % 16 and c.weights[0].data_ptr() % 16
    c.check(kernel)


def largest_sum_operands(fill):
    """a and c0 hold the constant in the columns below N / 2 and the key of element g in the columns that READ those
    (pi_g maps halves to halves), so half of the outputs are sums of D (and G) products of the largest
    operands; every other column is random, so a wrong permutation still shows.  Every weight word is 2^W - 1.
    fill: "top" -- the constant is 2^W - 1, which the header accepts (any word) and mac multiplies exactly; "q-1" -- the
    largest residue of the word's own modulus"""
    def make(c):
        g, bits, n, M, L, D, KM = c.g, c.bits, c.n, c.M, c.L, c.D, c.KM
        rng = np.random.default_rng(D + c.G + bits)
        top = (1 << bits) - 1
        dt = g.np_dtype(bits)
        per_limb = (lambda ms: np.array([top if fill == "top" else q - 1 for q in ms], dtype=dt))
        a = any_words(g, rng, bits, D * c.count * M * n).reshape(D, c.count, M, n)
        a[..., :n // 2] = per_limb(c.qs)[None, None, :, None]
        c0 = any_words(g, rng, bits, c.count * L * n).reshape(c.count, L, n)
        c0[..., :n // 2] = per_limb(c.qs[:L])[None, :, None]
        keys = []
        for k in c.elts:
            src = g.automorphism_index_map(c.n_power, k, c.st["poly"])
            key = any_words(g, rng, bits, D * 2 * KM * n).reshape(D, 2, KM, n)
            key[..., src < n // 2] = per_limb(c.qs)[None, None, :, None]  # key_mod_count = M here
            keys.append(key.reshape(-1))
        weights = [np.full(M * n, top, dtype=dt) for _ in range(c.G)]
        return dict(a=a.reshape(-1), c0=c0.reshape(-1), keys=keys, weights=weights)
    return make


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kind", ["wide", "spread"])
@pytest.mark.parametrize("fill", ["top", "q-1"])
@pytest.mark.parametrize("L,K,alpha,G", [(63, 1, 1, 2), (3, 2, 2, 64)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_largest_sums_the_contract_allows(g, kernel, L, K, alpha, G, fill, kind, bits):
    """across digits: D = 63 products per three-word accumulator, M = 64 limbs; across elements: G = 64, for the sum 64
    products of the unreduced fold sum (below 3 q) with a weight word 2^W - 1 in the second pair of accumulators --
    "at most 64 terms leave the carry word at 64" (csrc/hoisted_rotation.hip)"""
    c = whole(g, bits, 6, L, K, alpha, kind, None, G, 1, host=largest_sum_operands(fill))
    assert c.D == (63 if L == 63 else 2)
    assert c.KM == c.M
    got, want = c.run(kernel, True, False, which="all")
    assert np.array_equal(got, want)
    if kernel == "sum":  # every fourth weight 1, and no weights at all
        for which in (3, None):
            got, want = c.run(kernel, True, True, which)
            assert np.array_equal(got, want), which


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_no_stray_writes_and_inputs_unmodified(g, kernel, bits):
    """out and the scratch inside larger sentinel-filled buffers, on the widest primes"""
    import torch
    G, count = 5, 3
    c = whole(g, bits, 7, 3, 2, 2, "wide", np.random.default_rng(bits), G, count)
    words_out, pad = (G if kernel == "rotate" else 1) * 2 * count * c.L * c.n, 64
    big_out = filled(bits, words_out + 2 * pad, value=0x5A5A5A5A)
    sbytes = c.plan.hoisted_scratch_bytes(count, G) if kernel == "rotate" else c.plan.hoisted_sum_scratch_bytes(count)
    big_scratch = torch.full((sbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big_scratch.data_ptr() % 256 == 0
    got, want = c.run(kernel, True, True, which=3, out=big_out[pad:pad + words_out],
                      scratch=big_scratch[256:256 + sbytes])
    assert np.array_equal(got, want)
    assert bool((big_out[:pad] == 0x5A5A5A5A).all()) and bool((big_out[pad + words_out:] == 0x5A5A5A5A).all())
    assert bool((big_scratch[:256] == 0xA5).all()) and bool((big_scratch[256 + sbytes:] == 0xA5).all())
    assert all(torch.equal(t, k) for t, k in zip((c.a, c.c0, *c.keys, *c.weights), c.keep)), "an input was modified"
