"""Shared by tests/test_gpu_bfv_rings.py: the case of one ring (the {q, b} and {q, p} stacks of relin3_utils.bases, both
plans, the batch_hint = 1 pair at u64 2^14), the auxiliary bases bfv_utils.aux_count has to return, the rule by which a
forward transform takes the four-polynomial tile at u64 2^16, the checked call that watches the library's counter of that
tile, and the inputs decode's noise maximum is probed with."""
import math

import numpy as np

from bfv_utils import make_plan as make_bfv_plan
from hoisted_exact import NARROW
from hoisted_utils import device_words, make_plan
from innerprod_utils import from_words
from relin3_utils import bases

N_POWERS = (13, 14, 15, 16)
T = {64: (1 << 40) + 15, 32: 65537}  # the plaintext moduli of the multiply family's small-ring tests
K_P, ALPHA = 2, 2
WIDTHS = {"default": None, "wide": "wide", "narrow": NARROW[64]}

# What bfv_utils.aux_count returns: the smallest K_b with B >= 2 t' N Q, worked out on the host from the primes alone
# (t' = terms x t for a plan that adds `terms` products).  (bits, kind, L, t') -> K_b at n_power 13, 14, 15, 16.
# u64 default, L = 3: Q < 2^177, so 2 t N Q < 2^(1 + 40 + 16 + 177) = 2^234 against 57 + 60 + 59 + 58 = 234 bits of four
# primes just below their powers of two -- the fifth prime arrives exactly where the size proof needs it
AUX = {(64, "default", 3, T[64]): (4, 4, 4, 5), (64, "default", 3, 2 * T[64]): (4, 4, 5, 5),
       (64, "default", 3, 65537): (4, 4, 4, 4), (64, "default", 3, 2 * 65537): (4, 4, 4, 4),
       (64, "default", 6, T[64]): (7, 7, 8, 8), (64, "default", 6, 2 * T[64]): (7, 8, 8, 8),
       (64, "default", 6, 65537): (7, 7, 7, 7),
       (64, "wide", 3, T[64]): (4, 4, 4, 4), (64, "wide", 3, 2 * T[64]): (4, 4, 4, 4),
       (64, "wide", 3, 65537): (4, 4, 4, 4),
       (64, "narrow", 3, T[64]): (None, None, None, 5), (64, "narrow", 3, 2 * T[64]): (None, None, None, 5),
       (32, "default", 3, 65537): (5, 5, 5, 5), (32, "default", 3, 2 * 65537): (5, 5, 5, 5),
       (32, "default", 6, 65537): (8, 8, 8, 8), (32, "default", 6, 2 * 65537): (8, 8, 8, 8),
       (32, "wide", 3, 65537): (5, 5, 5, 5), (32, "wide", 3, 2 * 65537): (5, 5, 5, 5)}


def expected_aux(bits, kind, L, t_all, n_power):
    return AUX[(bits, kind, L, t_all)][n_power - 13]


class Setup:
    """one case: the ring's first L primes, K_b auxiliary primes behind them (asserted against AUX), K_p = 2 special
    primes behind those; a BfvMultiplyPlan of plaintext modulus t whose auxiliary base holds `terms` products and a
    KeySwitchPlan with alpha = 2.  At u64 2^14 a second pair built with batch_hint = 1, whose transforms take other
    tiles; at u64 2^16 on primes below 62 bits the forward transforms have the four-polynomial tile (p4)"""

    def __init__(self, g, bits, n_power, kind, L=3, t=None, terms=1):
        t = T[bits] if t is None else t
        self.g, self.bits, self.n_power, self.n, self.L, self.t, self.kind = g, bits, n_power, 1 << n_power, L, t, kind
        self.full, self.st_b, self.st_p, self.K_b = bases(g, bits, n_power, L, t * terms, K_p=K_P, widths=WIDTHS[kind])
        assert self.K_b == expected_aux(bits, kind, L, t * terms, n_power), ("aux_count", self.K_b)
        self.M_b, self.M_p = L + self.K_b, L + K_P
        self.qs, self.qb, self.qp = self.st_p["moduli"][:L], self.st_b["moduli"], self.st_p["moduli"]
        assert self.qb[:L] == self.qs and not set(self.qb[L:]) & set(self.qp[L:])
        self.Q = math.prod(self.qs)
        hints = ({}, {"batch_hint": 1}) if (bits, n_power) == (64, 14) else ({},)
        self.bfvs = [make_bfv_plan(g, self.st_b, L, t, n_power, bits, **kw) for kw in hints]
        self.kss = [make_plan(g, self.st_p, L, ALPHA, n_power, bits, **kw) for kw in hints]
        self.bfv, self.ks = self.bfvs[0], self.kss[0]
        assert self.bfv.b_count == self.K_b and self.bfv.max_terms >= terms
        self.D = self.ks.digits
        assert self.D == -(-L // ALPHA)
        self.p4 = bits == 64 and n_power == 16 and kind in ("default", "narrow")

    def cases(self, base):
        """the ring's MergeCases of a base, "q", "b" (the full base {q, b}) or "p" ({q, p}): what the exact references
        take where hoisted_exact.host_cases would be built a second time"""
        L, K_b = self.L, self.K_b
        idx = {"q": range(L), "b": range(L + K_b), "p": list(range(L)) + list(range(L + K_b, L + K_b + K_P))}[base]
        return [self.full.cases[i] for i in idx]


def p4_groups(*per_modulus):
    """lazy_launch.hpp: a forward u64 transform at 2^16 runs its last pass on the four-polynomial tile exactly when its
    polynomials are whole groups of four per modulus, in one launch of that tile.  per_modulus: the polynomials per
    modulus of every forward transform of a call (0: the transform does not run); returns the launches to expect"""
    return sum(p > 0 and p % 4 == 0 for p in per_modulus)


def p4_multiply(U, count, output_ntt):
    """bfv_multiply.cuh, "What runs": ONE full-base NTT over 2 U count M polynomials (U distinct operands: 2 for a
    product, 1 for a squaring), [ONE q-base NTT over 3 count L]"""
    return p4_groups(2 * U * count, 3 * count if output_ntt else 0)


def p4_relinearize(D, count, output_ntt):
    """key_switch.cuh: the full-base NTT of the D count M digits, [the q-base NTT over 2 count L]"""
    return p4_groups(D * count, 2 * count if output_ntt else 0)


def p4_multiply_relinearize(U, D, count, output_ntt):
    """steps 1 to 5 of multiply (no closing NTT of its own), then relinearize's coefficient path"""
    return p4_groups(2 * U * count) + p4_relinearize(D, count, output_ntt)


def run_checked(s, eligible, call, outs, wants, what, prefill=True):
    """call(i) on every plan pair i of the setup, every tensor of outs against its tensor of wants.  On the rings of the
    four-polynomial tile the library's launch counter of that tile moves by exactly `eligible`, the number of eligible
    forward transforms of the call, with the hook contig_p4 at 1; eligible calls run again with the hook at 0: the counter
    stays and the words are the same.  Returns the counter's movement with the hook at 1"""
    import torch
    g, moved_on = s.g, 0
    try:
        for i in range(len(s.bfvs)):
            for hook in (("1", "0") if s.p4 and eligible else ("1",)):
                if s.p4:
                    g.set_test_hook("contig_p4", hook)
                if prefill:
                    for o in outs:
                        o.fill_(-1)
                before = g.contig_p4_launches() if s.p4 else 0
                call(i)
                torch.cuda.synchronize()
                if s.p4:
                    moved = g.contig_p4_launches() - before
                    assert moved == (eligible if hook == "1" else 0), (what, "contig_p4=" + hook, eligible, moved)
                    moved_on = moved if hook == "1" else moved_on
                for k, (o, w) in enumerate(zip(outs, wants)):
                    assert torch.equal(o, w), (what, "output %d" % k, "plan %d" % i, "contig_p4=" + hook)
    finally:
        if s.p4:
            g.set_test_hook("contig_p4", "1")
    return moved_on


def small_device(x, offset=0):
    """int32 values -> a device tensor, `offset` words off 16-byte alignment"""
    import torch
    t = torch.zeros(x.size + offset, dtype=torch.int32, device="cuda:0")
    t[offset:] = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to("cuda:0")
    return t[offset:]


def object_words(g, x, bits, offset=0):
    """an object array of words -> a device tensor"""
    return device_words(g, np.ascontiguousarray(x.astype(np.uint64).astype(g.np_dtype(bits)).reshape(-1)), offset)


def host(g, t, shape):
    return from_words(g.to_host(t), shape)


def zeros_bytes(nbytes):
    import torch
    return torch.zeros(max(256, nbytes), dtype=torch.uint8, device="cuda:0")


# ------------------------------------------------------------------------------------------ decode's noise maximum
def decode_tiles(bits, n_power, aligned):
    """relin_grid: 256 lanes per tile, a lane owns a 16-byte group of columns, one column off 16-byte alignment"""
    V = (16 // (bits // 8)) if aligned else 1
    return max(1, (1 << n_power) // (256 * V))


def noisy_phase(rng, Q, t, n, stacks, unit):
    """x = round-half-up(Q m / t) + e per column with |e| <= 4 unit, in steps of unit / 1024: Python integers
    [stacks][N]"""
    m = rng.integers(0, t, size=(stacks, n))
    e = rng.integers(-4096, 4097, size=(stacks, n))
    x = np.empty((stacks, n), dtype=object)
    for k in range(stacks):
        x[k] = [((2 * Q * int(a) + t) // (2 * t) + (int(b) * unit >> 10)) % Q for a, b in zip(m[k], e[k])]
    return x


def plant(x, Q, t, stack, col, e):
    """move column `col` of `stack` by e more"""
    x[stack, col] = (int(x[stack, col]) + e) % Q


def limbs(x, qs):
    """integers [stacks][N] -> residues [stacks][L][N]"""
    return np.stack([x % q for q in qs], axis=1)


def sparse_product(m1, idx, val, t):
    """m1 m2 mod (t, X^N + 1) for m2 = sum_k val[k] X^idx[k] in Python integers: one shifted add per nonzero term"""
    n = len(m1)
    m1 = np.array([int(v) for v in m1], dtype=object)
    out = np.zeros(n, dtype=object)
    for k, c in zip(idx, val):
        k = int(k)
        out = out + int(c) * (np.concatenate([-m1[n - k:], m1[:n - k]]) if k else m1)
    return out % t
