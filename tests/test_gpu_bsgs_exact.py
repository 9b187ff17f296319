"""KeySwitchPlan.linear_transform_bsgs on the MI355X against the exact-integer reference of tests/bsgs_exact.py (pinned on
its own by tests/test_bsgs_exact_host.py): no GPU call on the expected side, array_equal on every output word.  Rings of
the widest primes Modulus<T> accepts, found from the top ("wide") and spread over the eighth below 2^(W-2) ("spread":
hoisted_utils.spread_factors says why the top alone does not reach the edge of the fold), and one ring of 45- / 20-bit
primes for contrast; a, c0, c1, the weights AND the keys of arbitrary words with 0, 2^W - 1, q - 1 and q planted (the
header reads every one of them modulo q_m); several steps without a key interleaved with keyed ones on both axes; the
largest sums the accumulators are promised to hold.  Each test prints what its host reference took."""
import time

import numpy as np
import pytest

from bsgs_exact import exact_bsgs_acc, exact_linear_transform_bsgs
from bsgs_utils import bsgs_elements, bsgs_scratch, with_absent
from hoisted_exact import NARROW, finish, transform
from hoisted_utils import any_words, device_words, filled, make_plan, ring
from innerprod_utils import from_words, words
from rescale_exact import finish_rescale

pytestmark = pytest.mark.gpu


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
    """one plan with its operands on the host (numpy words, and as Python integers) and on the device: n1 + n2 keys and
    n2 x n1 weights; which steps go without a key is chosen per run"""

    def __init__(self, g, full, limbs, L, alpha, bits, rng, n1, n2, count, host=None, **plan_kw):
        self.g, self.bits, self.L, self.alpha, self.n1, self.n2, self.count = g, bits, L, alpha, n1, n2, count
        self.st = full.sub(limbs)
        self.cases = [full.cases[i] for i in limbs]
        self.qs, self.n_power, self.n = self.st["moduli"], full.n_power, full.n
        self.plan = make_plan(g, self.st, L, alpha, full.n_power, bits, **plan_kw)
        self.key_limbs, self.R = plan_kw.get("key_limbs"), plan_kw.get("rescale_limbs", 0)
        self.M, self.D, self.KM = len(limbs), self.plan.digits, plan_kw.get("key_mod_count", len(limbs))
        self.belts, self.gelts = bsgs_elements(g, full.n_power, n1), bsgs_elements(g, full.n_power, n2)
        M, D, KM, n = self.M, self.D, self.KM, self.n
        if host is None:
            host = dict(a=any_words(g, rng, bits, D * count * M * n, self.qs),
                        c0=any_words(g, rng, bits, count * L * n, self.qs[:L]),
                        c1=any_words(g, rng, bits, count * L * n, self.qs[:L]),
                        bkeys=[any_words(g, rng, bits, D * 2 * KM * n, full.moduli) for _ in range(n1)],
                        gkeys=[any_words(g, rng, bits, D * 2 * KM * n, full.moduli) for _ in range(n2)],
                        weights=[[any_words(g, rng, bits, M * n, self.qs) for _ in range(n1)] for _ in range(n2)])
        else:
            host = host(self)
        self.a, self.c0, self.c1 = (device_words(g, host[k]) for k in ("a", "c0", "c1"))
        self.bkeys, self.gkeys = [device_words(g, k) for k in host["bkeys"]], [device_words(g, k) for k in host["gkeys"]]
        self.weights = [[device_words(g, w) for w in row] for row in host["weights"]]
        self.inputs = [self.a, self.c0, self.c1, *self.bkeys, *self.gkeys, *(w for row in self.weights for w in row)]
        self.keep = [t.clone() for t in self.inputs]
        self.h_a = from_words(host["a"], (D, count, M, n))
        self.h_c0, self.h_c1 = from_words(host["c0"], (count, L, n)), from_words(host["c1"], (count, L, n))
        self.h_bkeys = [from_words(k, (D, 2, KM, n)) for k in host["bkeys"]]
        self.h_gkeys = [from_words(k, (D, 2, KM, n)) for k in host["gkeys"]]
        self.h_weights = [[from_words(w, (M, n)) for w in row] for row in host["weights"]]
        self.host_seconds = 0.0

    def check(self, nulls=None, absent=True, c0s=(False, True), ntts=(False, True)):
        """c0 absent / present x output_ntt off / on.  nulls: per c0 variant the (baby, giant) sets of steps that go
        WITHOUT a key, at element 1; by default one per axis at a position that moves with the variant, one of them past
        the end (no such step on that axis), as test_gpu_bsgs.check_against_the_composition places them.  absent: one
        absent weight in every row, at a column that moves with the row and the variant (bsgs_utils.with_absent)"""
        import torch
        g, plan, bits, n1, n2, count = self.g, self.plan, self.bits, self.n1, self.n2, self.count
        keep = self.L - self.R
        call = plan.linear_transform_bsgs_rescale if self.R else plan.linear_transform_bsgs
        scratch = bsgs_scratch(plan, count, n1, n2)
        for i, with_c0 in enumerate(c0s):
            bnull, gnull = nulls[i] if nulls is not None else ({i % (n1 + 1)}, {(i + 1) % (n2 + 1)})

            def placed(keys, elts, null):
                return ([None if j in null else k for j, k in enumerate(keys)],
                        [1 if j in null else e for j, e in enumerate(elts)])
            bk, be = placed(self.bkeys, self.belts, bnull)
            gk, ge = placed(self.gkeys, self.gelts, gnull)
            h_bk, h_gk = placed(self.h_bkeys, self.belts, bnull)[0], placed(self.h_gkeys, self.gelts, gnull)[0]
            w, h_w = (with_absent(self.weights, i), with_absent(self.h_weights, i)) if absent else \
                (self.weights, self.h_weights)
            t0 = time.perf_counter()
            acc = exact_bsgs_acc(g, self.cases, self.L, self.alpha, bits, self.h_a, self.h_c0 if with_c0 else None,
                                 self.h_c1, h_bk, be, h_gk, ge, h_w, self.key_limbs)
            # the accumulators serve both outputs; what follows is exact_linear_transform_bsgs's own ending
            if self.R:  # finish_rescale takes the stack in coefficient form
                acc = transform(self.cases, acc.reshape(-1, self.M, self.n), True).reshape(acc.shape)
            self.host_seconds += time.perf_counter() - t0
            for output_ntt in ntts:
                t0 = time.perf_counter()
                want = finish_rescale(self.cases, self.L, self.R, acc, bits, output_ntt) if self.R else \
                    finish(self.cases, self.L, acc, bits, output_ntt)
                if i == 0 and output_ntt == ntts[-1]:  # once per case: the words of the whole reference call
                    assert np.array_equal(want, exact_linear_transform_bsgs(
                        g, self.cases, self.L, self.alpha, bits, self.h_a, self.h_c0 if with_c0 else None, self.h_c1,
                        h_bk, be, h_gk, ge, h_w, output_ntt, self.key_limbs, self.R))
                self.host_seconds += time.perf_counter() - t0
                assert want.shape == (2, count, keep, self.n)
                out = filled(bits, want.size)
                call(self.a, self.c0 if with_c0 else None, self.c1, bk, be, gk, ge, w, out, count, output_ntt, scratch)
                torch.cuda.synchronize()
                assert np.array_equal(g.to_host(out), words(g, want, bits)), \
                    (n1, n2, count, sorted(bnull), sorted(gnull), with_c0, output_ntt)
        assert all(torch.equal(t, k) for t, k in zip(self.inputs, self.keep)), "an input was modified"
        return self.host_seconds


def whole(g, bits, n_power, L, K, alpha, kind, rng, n1, n2, count, poly=None, **kw):
    M = L + K
    return Case(g, the_ring(g, bits, n_power, max(M, 8), kind, poly), list(range(M)), L, alpha, bits, rng, n1, n2, count,
                **kw)


def report(what, t0, host):
    print("%s: %.1f s, of which %.1f s the host reference" % (what, time.perf_counter() - t0, host))


COMBOS = [(3, 2, 3), (1, 3, 1), (4, 1, 3)]
RINGS_AND_SIZES = [("wide", 5), ("wide", 6), ("wide", 7), ("spread", 6), ("spread", 7)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kind,n_power", RINGS_AND_SIZES)
@pytest.mark.parametrize("L,K,alpha", [(3, 2, 2), (6, 2, 2)])
def test_every_output_word_with_chunks_of_64_slots(g, chunk6, L, K, alpha, kind, n_power, bits):
    """n_power 5: below a chunk, lanes without a slot; 6: one chunk exactly; 7: two chunks, the source chunk differs per
    giant step"""
    t0, host = time.perf_counter(), 0.0
    rng = np.random.default_rng(1000 * n_power + 10 * L + bits)
    for n1, n2, count in COMBOS:
        host += whole(g, bits, n_power, L, K, alpha, kind, rng, n1, n2, count).check()
    report("every word, %s 2^%d L=%d u%d" % (kind, n_power, L, bits), t0, host)


INTERLEAVED = [
    # n1, n2, the baby steps without a key, the giant steps without a key
    (5, 4, {0, 2}, {1, 3}),   # [None, key, None, key, key] x [key, None, key, None]
    (3, 2, {0, 1, 2}, {1}),   # no baby key at all
    (3, 3, {1}, {0, 1, 2}),   # no giant key at all
]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n1,n2,bnull,gnull", INTERLEAVED, ids=["interleaved", "no-baby-key", "no-giant-key"])
def test_several_steps_without_a_key_interleaved_with_keyed_ones(g, chunk6, bits, n1, n2, bnull, gnull):
    """the launcher moves the keyed steps first on both axes and permutes the weight table with them; here more than one
    step moves and keyed steps stand between them, every weight is different and one per row is absent, so a weight that
    lands in another place changes words.  The keyed elements of the first shape are (k, k', k): a duplicate"""
    t0 = time.perf_counter()
    c = whole(g, bits, 7, 3, 2, 2, "spread", np.random.default_rng(n1 + n2 + bits), n1, n2, 2)
    if n1 == 5:
        c.belts = [1, c.belts[0], 1, c.belts[1], c.belts[0]]
    host = c.check(nulls=[(bnull, gnull), (bnull, gnull)])
    report("interleaved (%d, %d) u%d" % (n1, n2, bits), t0, host)


@pytest.mark.parametrize("bits", [64, 32])
def test_one_narrow_ring(g, chunk6, bits):
    """primes of 45 / 20 bits: far from every edge of the word, the same words expected"""
    t0 = time.perf_counter()
    host = whole(g, bits, 7, 3, 2, 2, "narrow", np.random.default_rng(45 + bits), 3, 2, 3).check()
    report("narrow u%d" % bits, t0, host)


@pytest.mark.parametrize("bits", [64, 32])
def test_one_cyclic_ring(g, chunk6, bits):
    """a plan built with X_N_minus: elements reduced mod N, the cyclic slot order"""
    t0 = time.perf_counter()
    host = whole(g, bits, 6, 3, 2, 2, "wide", np.random.default_rng(6 + bits), 3, 2, 3, poly=g.X_N_minus).check()
    report("cyclic u%d" % bits, t0, host)


@pytest.mark.parametrize("bits", [64, 32])
def test_a_lower_level_plan_reads_the_full_level_keys_in_place(g, chunk6, bits):
    """L = 4 of keys built for 6 + 2 limbs: key_mod_count = 8, key_limbs = [0, 1, 2, 3, 6, 7]"""
    t0 = time.perf_counter()
    limbs = [0, 1, 2, 3, 6, 7]
    full = the_ring(g, bits, 7, 8, "spread")
    c = Case(g, full, limbs, 4, 2, bits, np.random.default_rng(bits), 3, 2, 3, key_mod_count=8, key_limbs=limbs)
    report("lower level u%d" % bits, t0, c.check())


@pytest.mark.parametrize("bits", [64, 32])
def test_the_automatic_chunk(g, bits):
    t0 = time.perf_counter()
    n_power = 9
    c = whole(g, bits, n_power, 6, 2, 2, "wide", np.random.default_rng(9 + bits), 3, 2, 2)
    assert g.keyswitch_hoist_sum_chunk(bits, c.D, n_power) > 6
    report("automatic chunk u%d" % bits, t0, c.check())


@pytest.mark.parametrize("bits,R", [(64, 1), (32, 2)])
def test_rescale(g, chunk6, bits, R):
    """linear_transform_bsgs_rescale against the reference ending in rescale_exact.finish_rescale"""
    t0 = time.perf_counter()
    c = whole(g, bits, 7, 4, 2, 2, "wide", np.random.default_rng(R + bits), 3, 2, 2, rescale_limbs=R)
    assert c.plan.kept_count == 4 - R
    report("rescale u%d R=%d" % (bits, R), t0, c.check())


def largest_sum_operands(fill):
    """test_gpu_hoisted_exact.largest_sum_operands' planting for this call: a, c0 and c1 hold the constant in the columns
    below N / 2 and the key of every step in the columns that READ those under its element (pi maps halves to halves),
    so half of the outputs are sums of D products of the largest operands per step; every other column is random, so a
    wrong permutation still shows.  Every weight word is 2^W - 1.  fill: "top" -- the constant is 2^W - 1, which the
    header accepts (any word) and mac multiplies exactly; "q-1" -- the largest residue of the word's own modulus"""
    def make(c):
        g, bits, n, M, L, D, KM, count = c.g, c.bits, c.n, c.M, c.L, c.D, c.KM, c.count
        rng = np.random.default_rng(D + c.n1 + 3 * c.n2 + bits)
        top = (1 << bits) - 1
        dt = g.np_dtype(bits)
        per_limb = (lambda ms: np.array([top if fill == "top" else q - 1 for q in ms], dtype=dt))
        a = any_words(g, rng, bits, D * count * M * n).reshape(D, count, M, n)
        a[..., :n // 2] = per_limb(c.qs)[None, None, :, None]
        cs = []
        for _ in range(2):
            x = any_words(g, rng, bits, count * L * n).reshape(count, L, n)
            x[..., :n // 2] = per_limb(c.qs[:L])[None, :, None]
            cs.append(x.reshape(-1))

        def key(k):
            src = g.automorphism_index_map(c.n_power, k, c.st["poly"])
            x = any_words(g, rng, bits, D * 2 * KM * n).reshape(D, 2, KM, n)
            x[..., src < n // 2] = per_limb(c.qs)[None, None, :, None]  # key_mod_count = M here
            return x.reshape(-1)
        weights = [[np.full(M * n, top, dtype=dt) for _ in range(c.n1)] for _ in range(c.n2)]
        return dict(a=a.reshape(-1), c0=cs[0], c1=cs[1], bkeys=[key(k) for k in c.belts],
                    gkeys=[key(k) for k in c.gelts], weights=weights)
    return make


LARGEST = [
    # (L, K, alpha), n1, n2, baby steps without a key, giant steps without a key
    ((3, 2, 2), 64, 4, set(), {3}),    # 64 products of a residue with 2^W - 1 per weighted-sum accumulator
    ((3, 2, 2), 4, 64, {0}, {63}),     # 63 keyed giant steps and one without: 64 words below 3 q across g
    ((63, 1, 1), 2, 2, {0}, {1}),      # D = 63 digits inside hoist_term of both kernels, M = 64
]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("kind", ["wide", "spread"])
@pytest.mark.parametrize("fill", ["top", "q-1"])
@pytest.mark.parametrize("shape,n1,n2,bnull,gnull", LARGEST, ids=["n1-64", "n2-64", "D-63"])
def test_the_largest_sums_the_contract_allows(g, shape, n1, n2, bnull, gnull, fill, kind, bits):
    """"at most 64 terms leave the carry word at 64" (bsgs_weighted_sum) and "at most 64 additions of words" of unreduced
    terms below 3 q (inner_product_galois_giant), csrc/hoisted_rotation.hip: the limits of the header, every weight
    present with every word 2^W - 1, the operands at their largest in half of the columns"""
    t0 = time.perf_counter()
    L, K, alpha = shape
    c = whole(g, bits, 6, L, K, alpha, kind, None, n1, n2, 1, host=largest_sum_operands(fill))
    assert c.D == (63 if L == 63 else 2) and c.KM == c.M
    host = c.check(nulls=[(bnull, gnull)], absent=False, c0s=(True,))
    report("largest sums %s (%d, %d) %s %s u%d" % (shape, n1, n2, fill, kind, bits), t0, host)
