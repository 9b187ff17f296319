"""BfvMultiplyPlan.multiply_sum without a GPU (include/gpuntt/rns/bfv_multiply.cuh): the definition (bfv_sum_exact)
against the ideal value round(t sum D / Q) in Python integers alone, max_terms against Python integers, the refusals that
need no device, and the text of bfv_tensor_sum on CPU threads under AddressSanitizer and UBSan
(tests/cpp/emulate_bfv_sum.cpp)."""
import math

import numpy as np
import pytest

from bfv_exact import exact_extend, exact_scale_round, ideal, in_band, integer_tensor, representatives
from bfv_sum_exact import MAX_TERMS, exact_tensor_sum, rounding_bound, slots_of
from bfv_sum_utils import run_sum_emulator
from bfv_utils import aux_count
from hoisted_exact import WIDE, host_cases
from innerprod_utils import from_words, random_words


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def sum_bases(bits, n_power, L, t, terms, spare=8):
    """NTT primes of the widest widths: the q-base and the smallest auxiliary base with B >= 2 terms t N Q"""
    mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], 2 * L + spare)]
    K = aux_count(mods, L, t * terms, 1 << n_power)
    return mods[:L], mods[L:L + K]


def rand_mod(rng, Q):
    return sum(int(rng.integers(0, 1 << 62)) << (62 * i) for i in range(Q.bit_length() // 62 + 2)) % Q


# (bits, L, n_power, t, count, terms as (x, y) operand indices): a squaring, a vector shared by every term, a pair twice
DEFINITION = [(32, 2, 2, 257, 1, [(0, 1)]), (64, 2, 3, 65537, 1, [(0, 0), (0, 1)]),
              (64, 3, 2, (1 << 40) + 15, 2, [(0, 1), (0, 2), (0, 3)]), (32, 3, 1, 65537, 1, [(0, 1), (2, 3), (0, 1)]),
              (64, 1, 2, 257, 1, [(i, i + 1) for i in range(8)])]


@pytest.mark.parametrize("bits,L,n_power,t,count,pairs", DEFINITION)
def test_the_definition_is_the_rounded_scaled_sum_of_tensors(bits, L, n_power, t, count, pairs):
    """Python integers alone: extend of every distinct operand, the integer tensors D_t of the representatives it chose,
    the residues of sum_t D_t in the full base (what step 2 of the definition holds: it is exact modulo every m_m),
    scale_round -- against round(t sum D / Q) mod q_i at every coefficient.  The seeds keep every coefficient outside
    step 2's rounding band: the count of band hits is asserted to be zero, so the equality is unconditional here"""
    n, terms = 1 << n_power, len(pairs)
    qs, bs = sum_bases(bits, n_power, L, t, terms)
    Q, B = math.prod(qs), math.prod(bs)
    assert B >= 2 * terms * t * n * Q
    rng = np.random.default_rng(bits + L + n_power + terms)
    reps, fulls = [], []
    for _ in range(1 + max(max(p) for p in pairs)):
        v = np.array([rand_mod(rng, Q) for _ in range(2 * count * n)], dtype=object).reshape(2 * count, n)
        full = exact_extend(qs, bs, np.moveaxis(np.stack([v % q for q in qs]), 0, 1), bits)
        rep = representatives(qs, bs, full)
        assert all(abs(int(r)) * (1 << bits) <= Q * ((1 << (bits - 1)) + 3 * L) for r in rep.reshape(-1))
        reps.append(rep.reshape(2, count, n))
        fulls.append(full.reshape(2, count, L + len(bs), n))
    D = sum(integer_tensor(reps[a], reps[b]) for a, b in pairs).reshape(3 * count, n)
    assert all(2 * t * abs(int(d)) <= B * Q for d in D.reshape(-1)), "the size proof: |t sum D / Q| <= B / 2"
    mods = qs + bs
    # in coefficient form the pointwise sum of step 2 is the residue of the integer sum: the transforms are linear
    stack = np.moveaxis(np.stack([D % m for m in mods]), 0, 1)
    out = exact_scale_round(qs, bs, t, stack, bits)
    band = in_band(qs, bs, t, stack, bits)
    assert int(band.sum()) == 0, "a coefficient of this seed lies in the rounding band: choose another seed"
    want = np.moveaxis(np.stack([ideal(t, D, Q) % q for q in qs]), 0, 1)
    assert np.array_equal(out, want)
    # and the bound of the header against the separate roundings, which holds without its band term here
    parts = sum(ideal(t, integer_tensor(reps[a], reps[b]).reshape(3 * count, n), Q) for a, b in pairs)
    diff = [abs(int(d)) for d in (ideal(t, D, Q) - parts).reshape(-1)]
    assert max(diff) <= rounding_bound(terms, bands=False), (max(diff), terms)
    # exact_tensor_sum on residues IS that sum, pointwise, whatever the form: checked on the extended words themselves
    e = np.stack(fulls)
    x_slot, y_slot = [a for a, _ in pairs], [b for _, b in pairs]
    d = exact_tensor_sum(mods, e, x_slot, y_slot)
    for m, q in enumerate(mods):
        ref = sum(e[a, 0, :, m] * e[b, 1, :, m] + e[a, 1, :, m] * e[b, 0, :, m] for a, b in pairs) % q
        assert np.array_equal(d[1, :, m], ref)


def test_slots_follow_first_appearance():
    a, b, c = (np.zeros(1, dtype=object) for _ in range(3))
    distinct, x_slot, y_slot = slots_of([a, b, a, c], [a, a, b, c])
    assert [id(v) for v in distinct] == [id(a), id(b), id(c)]
    assert x_slot == [0, 1, 0, 2] and y_slot == [0, 0, 1, 2]


@pytest.mark.parametrize("bits,t", [(64, 65537), (32, 257)])
def test_max_terms_against_python_integers(g, bits, t):
    """min(32, B // (2 t N Q)): 1 for the smallest base of one term, an interior value, and the cap"""
    L, n_power = 3, 5
    n = 1 << n_power
    mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], 2 * L + 8)]
    qs = mods[:L]
    Q = math.prod(qs)
    seen = set()
    for K in range(1, len(mods) - L + 1):
        bs = mods[L:L + K]
        want = min(MAX_TERMS, math.prod(bs) // (2 * t * n * Q))
        if want == 0:
            with pytest.raises(ValueError, match="Auxiliary base too small!"):
                g.bfv_max_terms(qs, bs, t, n_power, bits)
            continue
        assert g.bfv_max_terms(qs, bs, t, n_power, bits) == want, K
        seen.add(want)
    assert MAX_TERMS in seen
    # the values between.  max_terms needs no transform, so the ring size is free here: pick K and n_power for which
    # room = B // (2 N Q) is a word of at least 12 bits; then t = room // target makes the quotient exactly target
    bs, np_, room = next((mods[L:L + K], p, math.prod(mods[L:L + K]) // ((2 << p) * Q))
                         for K in range(1, len(mods) - L + 1) for p in range(1, 29)
                         if 1 << 12 <= math.prod(mods[L:L + K]) // ((2 << p) * Q) < 1 << bits)
    for target in range(1, 34):
        tt = room // target
        want = math.prod(bs) // (2 * tt * (1 << np_) * Q)
        assert want == target  # target^2 < 2^12 <= room
        assert g.bfv_max_terms(qs, bs, tt, np_, bits) == min(MAX_TERMS, want), target
        # one more than t: the quotient at a threshold falls by one, in exact integers
        below = math.prod(bs) // (2 * (tt + 1) * (1 << np_) * Q)
        if below >= 1:
            assert g.bfv_max_terms(qs, bs, tt + 1, np_, bits) == min(MAX_TERMS, below), target
        seen.add(min(MAX_TERMS, want))
    assert set(range(1, MAX_TERMS + 1)) <= seen


def test_refusals_that_need_no_device(g):
    bits, L, n_power, t = 64, 3, 5, 65537
    mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], 2 * L + 4)]
    qs, bs = mods[:L], mods[L:2 * L + 1]
    refused = [lambda: g.bfv_max_terms(qs, bs[:1], t, n_power, bits),              # B < 2 t N Q
               lambda: g.bfv_max_terms(qs, bs, t, 0, bits), lambda: g.bfv_max_terms(qs, bs, t, 29, bits),
               lambda: g.bfv_max_terms(qs, bs, 1, n_power, bits),                  # t < 2
               lambda: g.bfv_max_terms([], bs, t, n_power, bits), lambda: g.bfv_max_terms(qs, [], t, n_power, bits),
               lambda: g.bfv_max_terms(qs, bs[:-1] + [qs[0]], t, n_power, bits)]   # not coprime
    for f in refused:
        with pytest.raises(ValueError):
            f()
    sb = g.BfvMultiplyPlan.sum_scratch_bytes
    plan = object.__new__(g.BfvMultiplyPlan)  # the static size needs no plan on a device: only the shape
    plan.bits, plan.q_count, plan.b_count, plan.n_power = bits, L, len(bs), n_power
    M = L + len(bs)
    poly = (3 << n_power) * 8

    def want(count, operands):
        return poly // 3 * count * M * 2 * max(operands, 2) + poly // 3 * count * L * 2
    assert sb(plan, 3, 1) == sb(plan, 3, 2) == want(3, 2) == g.BfvMultiplyPlan.scratch_bytes(plan, 3)
    assert sb(plan, 3, 5) == want(3, 5) and sb(plan, 1, 64) == want(1, 64) and sb(plan, 0, 3) == 0
    for count, operands in ((-1, 2), (1, 0), (1, 65), (1, -1)):
        with pytest.raises(ValueError):
            sb(plan, count, operands)
    plan._h = None  # nothing to destroy


# (bits, n_power, M, count, slots, off, terms as (x_slot, y_slot)).  N = 2 at u32 is below a group (the one-word loader),
# as is any region one word off alignment; N = 4 and N = 8 take the group loader; N = 2048 at u32 and 1024 at u64 have
# two column tiles (256 lanes of 4 / 2 columns).  terms 1, 2 and 32; a slot that is the x and the y of every term;
# slots 0 and 1 both read in the LAST term, after every other slot -- the planes the output goes over
ALL_SELF = [(0, 0)] * MAX_TERMS
LAST = [(2, 3), (3, 2), (2, 2), (0, 1)]
EMULATED = [(32, 1, 2, 1, 2, 0, [(0, 1)]), (32, 2, 3, 2, 4, 0, LAST), (32, 3, 2, 1, 2, 0, [(0, 1), (1, 0)]),
            (32, 3, 2, 3, 2, 1, [(0, 1), (1, 1)]), (64, 1, 2, 2, 2, 0, [(0, 0)]), (64, 2, 3, 1, 4, 0, LAST),
            (64, 3, 2, 2, 3, 1, [(0, 2), (2, 1)]), (64, 2, 2, 1, 2, 0, ALL_SELF), (32, 2, 2, 1, 2, 0, ALL_SELF),
            (64, 2, 2, 1, 2, 0, [(0, 1)] * MAX_TERMS), (32, 2, 2, 1, 64, 0, [(2 * i, 2 * i + 1) for i in range(32)]),
            (32, 11, 1, 2, 2, 0, [(1, 0), (0, 0)]), (64, 10, 1, 1, 3, 0, [(0, 1), (2, 0)])]


def test_the_kernels_text_on_cpu_threads_under_sanitizers(g, tmp_path):
    """every word of bfv_tensor_sum against bfv_sum_exact; the program itself reports a touched guard band or a changed
    word behind the three output planes.  Every input word is m_m - 1 or 0 in the ALL_SELF and 32-term cases on the widest
    primes of both widths (d1 takes 64 maximal products), any word elsewhere"""
    rng = np.random.default_rng(11)
    job, want = [len(EMULATED)], []
    for bits, n_power, M, count, slots, off, pairs in EMULATED:
        n, terms = 1 << n_power, len(pairs)
        mods = [c.q for c in host_cases(bits, n_power, WIDE[bits], M)]
        assert max(mods).bit_length() == max(WIDE[bits])
        top = (1 << bits) - 1
        if terms == MAX_TERMS:
            e = np.zeros((slots, 2, count, M, n), dtype=object)
            for m, q in enumerate(mods):
                e[:, :, :, m, :] = q - 1
            e[:, :, :, :, n - 1] = 0  # and a column of zeros
            if slots > 2:
                e[-1] = 0
        else:
            e = random_words(rng, (slots, 2, count, M, n), bits)
            for m, q in enumerate(mods):
                for k, v in enumerate((0, top, q - 1, q)):
                    e[k % slots, k % 2, -1, m, (k + m) % n] = v
        x_slot, y_slot = [a for a, _ in pairs], [b for _, b in pairs]
        job += [bits, n_power, M, count, slots, terms, off] + mods + x_slot + y_slot
        job += [int(v) for v in e.reshape(-1)]
        want.append(exact_tensor_sum(mods, e, x_slot, y_slot))
    got, printed = run_sum_emulator(tmp_path, np.array(job, dtype=np.uint64))
    lines = printed.splitlines()
    assert sum("vec=0" in ln for ln in lines) >= 3 and sum("vec=1" in ln for ln in lines) >= 8, printed
    assert any("tiles=2" in ln or "tiles=4" in ln for ln in lines), printed
    at = 0
    for case, w in zip(EMULATED, want):
        part = got[at:at + w.size]
        at += w.size
        assert np.array_equal(from_words(part, w.shape), w), case[:6]
    assert at == got.size
    # the widest sums really were maximal: 64 products of (m - 1)^2 in d1
    q = [c.q for c in host_cases(64, 2, WIDE[64], 2)][0]
    assert int(want[7][1, 0, 0, 0]) == 64 * (q - 1) ** 2 % q
