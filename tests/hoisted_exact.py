"""KeySwitchPlan.rotate_hoisted and rotate_hoisted_sum (include/gpuntt/rns/key_switch.cuh) restated in Python integers
(numpy object arrays: one Python int per word, as keyswitch_utils does).  No GPU call and none of the library's
arithmetic: the accumulators follow the header's formulas, pi_g comes from automorphism_index_map (pinned against
numpy's sigma by tests/test_galois_host.py), the transforms are the in-repo oracle's restated NTTCPU
(gpu_utils.oracle_batch) and the ModDown is keyswitch_utils.ref_mod_down.  Every step is defined word for word, so what
these functions return is compared with array_equal."""
import math
from types import SimpleNamespace

import numpy as np

from gpu_utils import distinct_factors_scaled, oracle_batch
from hoisted_utils import WIDE_WIDTHS as WIDE
from innerprod_utils import from_words
from keyswitch_utils import ref_mod_down
from oracle import oracle as O

NARROW = {64: (45,), 32: (20,)}  # one narrow ring for contrast with hoisted_utils.WIDE_WIDTHS


def host_cases(bits, n_power, widths, M, poly=O.X_N_plus):
    """M NTT primes of the widths (cycled) with the oracle's tables: what oracle_batch reads of a MergeCase, without a
    device"""
    P = O.Port(bits)
    return [SimpleNamespace(P=P, logn=n_power, n=1 << n_power, poly=poly, q=f[0], oprm=P.merge_params(n_power, poly, f))
            for f in distinct_factors_scaled([widths[i % len(widths)] for i in range(M)], n_power)]


def transform(cases, x, inverse):
    """NTTCPU::ntt / ::intt of x [...][len(cases)][N] (canonical object words), polynomial under its limb's modulus"""
    dt = cases[0].P.T
    flat = np.ascontiguousarray(x.astype(np.uint64).astype(dt).reshape(-1))
    return from_words(oracle_batch(cases, flat, inverse=inverse), x.shape)


def exact_u(g, qs, L, n_power, poly, a, c0, keys, elts, key_limbs=None):
    """u_g[c][r][m][j] = (sum_d a[d][r][m][pi_g(j)] key_g[d][c][limb(m)][j]
                          + [c = 0, m < L, c0 given] (P mod q_m) c0[r][m][pi_g(j)]) mod q_m, every word read modulo q_m.
    a [D][count][M][N], c0 [count][L][N] or None, keys: G arrays [D_key][2][key_mod_count][N]; returns
    u [G][2][count][M][N]"""
    D, count, M, n = a.shape
    P = math.prod(qs[L:])
    limbs = list(range(M)) if key_limbs is None else list(key_limbs)
    u = np.zeros((len(elts), 2, count, M, n), dtype=object)
    for i, k in enumerate(elts):
        src = g.automorphism_index_map(n_power, k, poly).astype(np.int64)
        for m, q in enumerate(qs):
            am = (a[:, :, m, :] % q)[:, :, src]  # [D][count][N], permuted
            for c in range(2):
                km = keys[i][:D, c, limbs[m], :] % q
                s = (am * km[:, None, :]).sum(axis=0)
                if c == 0 and m < L and c0 is not None:
                    s = s + (P % q) * (c0[:, m, :] % q)[:, src]
                u[i, c, :, m, :] = s % q
    return u


def exact_weighted_sum(qs, u, weights):
    """acc[c][r][m][j] = (sum_g w_g[m][j] u_g[c][r][m][j]) mod q_m; weights: None or a list of [M][N] arrays / None (a
    null weight is 1), any words, read modulo q_m"""
    G = u.shape[0]
    acc = np.zeros(u.shape[1:], dtype=object)
    for i in range(G):
        w = None if weights is None else weights[i]
        for m, q in enumerate(qs):
            wm = 1 if w is None else (w[m] % q)[None, None, :]
            acc[:, :, m, :] = acc[:, :, m, :] + u[i, :, :, m, :] * wm
    for m, q in enumerate(qs):
        acc[:, :, m, :] = acc[:, :, m, :] % q
    return acc


def finish(cases, L, acc, bits, output_ntt):
    """the plan's own steps after the accumulators: the full-base inverse transform, mod_down, the q-base forward
    transform when output_ntt.  acc [...][M][N] canonical -> [...][L][N]"""
    M, n = acc.shape[-2:]
    qs = [c.q for c in cases]
    x = transform(cases, acc.reshape(-1, M, n), True)
    out = ref_mod_down(qs[:L], qs[L:], x, bits)
    if output_ntt:
        out = transform(cases[:L], out, False)
    return out.reshape(acc.shape[:-2] + (L, n))


def exact_rotate_hoisted(g, cases, L, bits, a, c0, keys, elts, output_ntt, key_limbs=None):
    """out [G][2][count][L][N]"""
    c = cases[0]
    u = exact_u(g, [k.q for k in cases], L, c.logn, c.poly, a, c0, keys, elts, key_limbs)
    return finish(cases, L, u, bits, output_ntt)


def exact_rotate_hoisted_sum(g, cases, L, bits, a, c0, keys, elts, weights, output_ntt, key_limbs=None):
    """out [2][count][L][N]"""
    c = cases[0]
    qs = [k.q for k in cases]
    u = exact_u(g, qs, L, c.logn, c.poly, a, c0, keys, elts, key_limbs)
    return finish(cases, L, exact_weighted_sum(qs, u, weights), bits, output_ntt)
