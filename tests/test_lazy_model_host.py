"""CPU side of the lazy-arithmetic tests: the generated operands are the hard ones, the constants the header computes are
the documented ones, and the range planners keep every bound.  Uses the host-only modes of tests/cpp/lazy_arith_probe.hip
(lazy.hpp's own make_norm_const / norm_const_of / ct_plan / gs_plan, compiled from the header; no HIP call is made)."""
import subprocess

import pytest

import lazy_model as L
import lazy_probe_utils as U

# The (LIMIT, TB) pairs the kernels instantiate per direction: the Mod<...> specialisations at the end of the Mod64 and
# Mod32 sections of gpu-ntt_amd/csrc/lazy.hpp -- Mod<u64, 0 | 31 | 8 | 4>, Mod<u64, 4 | 0 | 8, VQ>, Mod<u32, 0 | 8>,
# Mod<u32, 0, VQ> (LIM 0 = 16 q in 64-bit words, 4 q in 32-bit words).  31 q is the forward-only family (host-side
# switch lim = 31): gs_plan is NOT used with LIMIT 31 -- test_gs_plan_is_not_for_limit_31.
FORWARD = {64: ((16, 4), (31, 4), (8, 4), (4, 2)), 32: ((4, 2), (8, 2))}
INVERSE = {64: ((16, 4), (8, 4), (4, 2)), 32: ((4, 2), (8, 2))}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return U.build_probe(str(tmp_path_factory.mktemp("lazy_probe_host") / "lazy_arith_probe"))


def host_mode(probe, tmp_path, mode, lines):
    path = str(tmp_path / (mode + ".txt"))
    with open(path, "w") as f:
        f.write("".join(" ".join(str(v) for v in ln) + "\n" for ln in lines))
    r = subprocess.run([probe, mode, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("family", list(L.FAMILIES))
def test_cases_reach_the_edges(family):
    """what keeps the device test from being vacuous, on the generator's output with the documented formulas"""
    fam = L.FAMILIES[family]
    moduli, c = U.family_cases(family)
    widths = sorted({bit for _, bit in moduli})
    assert widths == list(range(2, fam.max_bit + 1)), "a stated width without a modulus"
    assert c.ncase <= L.MAX_CASES and c.ncase % L.WAVE == 0 and c.nuni % L.WAVE == 0
    for q, bit in moduli:
        assert q & 1 and bit >= q.bit_length() and fam.lim * q < (1 << fam.W)
    if fam.W == 64:  # a modulus whose `bit` is over-stated sits in the family its stated width selects
        over = [(q, bit) for q, bit in moduli if bit == q.bit_length() + 1]
        assert any(q == (1 << (bit - 1)) - 107 for q, bit in over), over[:3]
    if not fam.vq:
        assert all(c.q[i] == c.qb[i // L.WAVE] and c.bit[i] == c.bitb[i // L.WAVE] for i in range(c.ncase))
    else:  # the mixed half really mixes: (nearly) every wave holds many moduli
        assert all(c.q[i] == c.qb[i // L.WAVE] for i in range(c.nuni))
        mixed = [len(set(c.q[b:b + L.WAVE])) for b in range(c.nuni, c.ncase, L.WAVE)]
        assert min(mixed) > L.WAVE // 2
    xs, short2_v, short2_u, t3q_v, t3q_u, tmax = {}, set(), set(), set(), set(), {}
    for i in range(c.nuni):
        q, bit, x = c.q[i], c.bit[i], c.x[i]
        xs.setdefault(bit, set()).add((q, x))
        assert 0 < c.w[i] < q and c.wp[i] == (c.w[i] << fam.W) // q
        if fam.W == 64:
            b = i // L.WAVE
            for w, wp, s2, t3 in ((c.w[i], c.wp[i], short2_v, t3q_v), (c.wu[b], c.wpu[b], short2_u, t3q_u)):
                t, short = L.documented_product(x, w, wp, q)
                assert 0 <= t < 4 * q and 0 <= short <= 2  # the header's [0, 4q) claim, on paper
                if short == 2:
                    s2.add(bit)
                if t >= 3 * q:
                    t3.add(bit)
                tmax[bit] = max(tmax.get(bit, 0), t)
    top = (1 << fam.W) - 1
    for q, bit in moduli:  # every edge word of every modulus: k q + d, k = 0 .. 32 (x = 0, 1, 2 among them), clipped
        for k in range(33):
            for d in (-2, -1, 0, 1, 2):
                assert (q, min(max(k * q + d, 0), top)) in xs[bit], "x = %d q %+d missing for q = %d" % (k, d, q)
        assert {(q, 0), (q, top), (q, top >> (fam.W // 2)), (q, top - (top >> (fam.W // 2)))} <= xs[bit]
    for bit in widths:
        have = xs[bit]
        for k in sorted(k for k in set(fam.ks) | set(fam.norms) if k <= fam.lim):  # (norm32: past the word at 60 bits)
            for q in (q for q, b in moduli if b == bit):
                assert (q, k * q - 1) in have and (q, k * q) in have, "x = %d q - 1 / %d q missing for q = %d" % (k, k, q)
                # csub_c<K> gets the COMPLEMENTS of the same words (the probe complements x), inside its domain x < 2 K q
                assert k * q <= top and L.csub_domain(k * q, k, q, fam.W) and L.csub_domain(k * q - 1, k, q, fam.W)
    if fam.W == 64:
        assert short2_v == set(widths) and short2_u == set(widths), "a width without a quotient that is 2 short"
        # T >= 3 q: for every width but 2.  q = 3 is the only modulus of 2 bits, and there T <= 8 < 3 q for every word:
        # w = 1 has wp = (2^64 - 1) / 3 with both halves c = (2^32 - 1) / 3, and T = (x1 - 3 floor(x1 c / 2^32)) + (x0 - 3
        # floor(x0 c / 2^32)), each term at most 3 (a mod 3 = 0 where the floor falls one short); w = 2 likewise with at most
        # 4 per term.  There the case set must hold that maximum, 3 q - 1.
        for s in (t3q_v, t3q_u):
            assert s | {2} == set(widths) and 2 not in s, "a width whose products do not reach 3 q"
        assert tmax[2] == 8


def test_norm_constants_are_the_documented_ones(probe, tmp_path):
    """make_norm_const / norm_const_of as compiled from the header = the record of the documented formulas, for every
    modulus of the generator; and the documented estimate with those records keeps reduce_2q's contract at the edges"""
    moduli = sorted({(L.FAMILIES[f].W, q, bit) for f in L.FAMILIES for q, bit in U.family_cases(f)[0]})
    assert any(L.make_norm_const(q, bit).M == 0xFFFFFFFF for W, q, bit in moduli if W == 64), "no capped M"
    assert {0, 1} <= {L.make_norm_const(q, bit).hi for W, q, bit in moduli if W == 64}
    assert any(L.make_norm_const(q, bit).sh == 0 for W, q, bit in moduli if W == 64)
    out = host_mode(probe, tmp_path, "norm", moduli)
    for (W, q, bit), got in zip(moduli, out):
        nc = L.make_norm_const(q, bit, W)
        assert [int(v) for v in got] == [W, q, bit, nc.sh, nc.c, nc.M, nc.hi]
        if W == 64 and bit > 61:
            assert nc == (0, 0, 0, 0)  # 62-bit moduli: LIMIT 4, normalised by conditional subtractions alone
            continue
        for k in range(33):
            for d in (-2, -1, 0, 1, 2):
                x = k * q + d
                if 0 <= x < min(32 * q, 1 << 64) and (W == 64 or x < (1 << 32)):
                    r = L.documented_reduce_2q(x, q, nc)
                    assert 0 <= r < 2 * q and (x - r) % q == 0, (W, q, bit, x, r)
        if W == 32:  # any word
            for x in (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFF0000, 0x0000FFFF, 0x80000000):
                assert 0 <= L.documented_reduce_2q(x, q, nc) < 2 * q


def exact_csub(b, k):
    """bound (units of q, exclusive) after `if (x >= k q) x -= k q` on x < b q; k = 0: none"""
    return b if k == 0 else max(min(b, k), b - k)


def test_range_planners_keep_every_bound(probe, tmp_path):
    """ct_plan / gs_plan, as compiled from the header, simulated with exact bounds for every input bound up to LIMIT"""
    combos = sorted({(lim, tb) for t in (FORWARD, INVERSE) for W in t for lim, tb in t[W]})
    lines = [(bu, bv, lim, tb) for lim, tb in combos for bu in range(1, lim + 1) for bv in range(1, lim + 1)]
    plans = {}
    for ln, got in zip(lines, host_mode(probe, tmp_path, "plan", lines)):
        v = [int(t) for t in got if t.lstrip("-").isdigit()]
        assert tuple(v[:4]) == ln
        plans[ln] = (v[4:6], v[6:11])
    for W in FORWARD:
        for lim, tb in FORWARD[W]:
            for bu in range(1, lim + 1):
                ku, out = plans[(bu, 1, lim, tb)][0]
                assert ku == 0 or bu <= 2 * ku  # the 32-bit min form is stated for x < 2 K q
                u = exact_csub(bu, ku)
                assert u + tb <= lim            # U + T stays below LIMIT q; V' = U - T + TB q > 0 lies below it too
                assert u + tb <= out <= lim     # both outputs within the stated bound, which the next stage may take
    for W in INVERSE:
        for lim, tb in INVERSE[W]:
            assert tb <= lim // 2               # the product V' is handed over as it is
            for bu in range(1, lim + 1):
                for bv in range(1, lim + 1):
                    ku, kv, c, ko, out_u = plans[(bu, bv, lim, tb)][1]
                    assert (ku == 0 or bu <= 2 * ku) and (kv == 0 or bv <= 2 * kv)
                    u, v = exact_csub(bu, ku), exact_csub(bv, kv)
                    assert c >= v               # U + c q - V cannot go negative
                    assert u + c <= lim         # ... and stays below LIMIT q
                    assert u + v <= lim         # the sum does not wrap
                    assert ko == 0 or u + v <= 2 * ko
                    assert exact_csub(u + v, ko) <= out_u <= lim // 2  # hand-over at or below LIMIT / 2


def test_gs_plan_is_not_for_limit_31(probe, tmp_path):
    """31 q is a forward-only range: gs_plan would hand over 16 > 31 / 2.  Harmless while no inverse kernel is
    instantiated with it -- INVERSE above has no 31, as lazy.hpp has no inverse Mod<u64, 31> user."""
    assert all(lim != 31 for W in INVERSE for lim, _ in INVERSE[W])
    (got,) = host_mode(probe, tmp_path, "plan", [(31, 31, 31, 4)])
    assert int(got[-1]) == 16 > 31 // 2
