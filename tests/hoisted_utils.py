"""Shared by the hoisted-rotation tests (KeySwitchPlan.rotate_hoisted, include/gpuntt/rns/key_switch.cuh): rings with
their tables, random operands, and the DEFINITION of rotate_hoisted as the composition of the public calls that existed
before it -- GPU_Automorphism_NTT, switch_digits, and the rotated c0 added to component 0."""
import numpy as np

from gpu_utils import MergeCase, distinct_factors_scaled

_rings = {}
DEFAULT_WIDTHS = {64: (60, 59, 58, 57), 32: (30, 29, 28, 27)}
# the top of what Modulus<T> accepts: 3 q < 2^W is all the kernels' bounds rest on
WIDE_WIDTHS = {64: (62, 61, 62, 60), 32: (30, 29, 30, 28)}


def tdtype(bits):
    import torch
    return torch.int64 if bits == 64 else torch.int32


def spread_factors(bits, M, logn):
    """(q, omega, psi) for M NTT primes of bits - 2 bits spread over the eighth below 2^(bits-2).  The primes a search
    from the top finds lie within ~2^(logn+10) of the power of two: there 2^W mod q and 2^2W mod q are tiny, the three-
    product fold puts all its weight on two terms and its sum never passes 2 q.  Only moduli further down drive the
    sum into [2^(W-1), 3 q), where a signed comparison or a lost top carry shows."""
    from gpu_utils import _is_probable_prime
    w, step, out = bits - 2, 1 << (logn + 1), []
    for i in range(M):
        q = ((1 << w) - ((1 << (w - 3)) * (i + 1)) // (M + 1)) // step * step + 1
        while not _is_probable_prime(q):
            q -= step
        assert q.bit_length() == w and all(q != f[0] for f in out)
        b = 2
        while True:
            psi = pow(b, (q - 1) >> (logn + 1), q)
            if pow(psi, 1 << logn, q) == q - 1:
                break
            b += 1
        out.append((q, psi * psi % q, psi))
    return out


class Ring:
    """M NTT primes of the given widths, cycled (below 2^(W-2), so that a sum of two residues, at most 2 q - 2 <
    2^(W-1), fits the signed torch type) with their tables for one (bits, n_power, reduction polynomial)"""

    def __init__(self, g, bits, n_power, M, poly, widths=None):
        if widths == "spread":
            factors = spread_factors(bits, M, n_power)
        else:
            widths = DEFAULT_WIDTHS[bits] if widths is None else tuple(widths)
            assert max(widths) <= bits - 2
            factors = distinct_factors_scaled([widths[i % len(widths)] for i in range(M)], n_power)
        self.cases = [MergeCase(g, bits, n_power, poly, f) for f in factors]
        n = 1 << n_power
        dt = g.np_dtype(bits)
        fwd, inv = np.zeros(M * n, dtype=dt), np.zeros(M * n, dtype=dt)
        for i, c in enumerate(self.cases):
            fwd[i * n:i * n + c.prm.root_of_unity_size] = c.prm.forward_table_device_order
            inv[i * n:i * n + c.prm.root_of_unity_size] = c.prm.inverse_table_device_order
        self.g, self.bits, self.n_power, self.n, self.M, self.poly = g, bits, n_power, n, M, poly
        self.moduli = [c.q for c in self.cases]
        self.n_inv = [c.prm.n_inv for c in self.cases]
        self.fwd, self.inv = g.to_device(fwd), g.to_device(inv)

    def sub(self, idx):
        """the stack of the moduli idx (a list of indices): values, device moduli, tables, n^-1 (host and device)"""
        import torch
        g, n = self.g, self.n
        t = torch.from_numpy(np.concatenate([np.arange(i * n, (i + 1) * n) for i in idx])).to("cuda:0")
        ninv = [self.n_inv[i] for i in idx]
        return dict(moduli=[self.moduli[i] for i in idx], poly=self.poly,
                    mods=g.modulus_array_to_device([self.cases[i].prm.modulus for i in idx], self.bits),
                    fwd=self.fwd[t].contiguous(), inv=self.inv[t].contiguous(), n_inv=ninv,
                    d_ninv=g.to_device(np.array(ninv, dtype=g.np_dtype(self.bits))))


def ring(g, bits, n_power, M=8, poly=None, widths=None):
    """widths: None (DEFAULT_WIDTHS), "wide" (WIDE_WIDTHS), "spread" (spread_factors) or a tuple of prime widths, cycled
    over the M primes"""
    poly = g.X_N_plus if poly is None else poly
    if widths != "spread":
        widths = DEFAULT_WIDTHS[bits] if widths is None else WIDE_WIDTHS[bits] if widths == "wide" else tuple(widths)
    key = (bits, n_power, M, poly, widths)
    if key not in _rings:
        _rings[key] = Ring(g, bits, n_power, M, poly, widths)
    return _rings[key]


def make_plan(g, st, L, alpha, n_power, bits, **kw):
    return g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, st["fwd"], st["inv"], st["n_inv"],
                           st["poly"], bits=bits, **kw)


def filled(bits, size, offset=0, value=-1):
    """a device tensor of `size` words of one value; offset: words by which the base pointer leaves 16-byte alignment"""
    import torch
    return torch.full((size + offset,), value, dtype=tdtype(bits), device="cuda:0")[offset:]


def device_words(g, w, offset=0):
    import torch
    t = torch.zeros(w.size + offset, dtype=tdtype(8 * w.dtype.itemsize), device="cuda:0")
    t[offset:] = g.to_device(w)
    return t[offset:]


def any_words(g, rng, bits, size, qs=()):
    """uniform words of the whole range (not residues), with 0, 2^W - 1 and q - 1 planted"""
    x = rng.integers(0, 1 << bits, size=size, dtype=np.uint64).astype(g.np_dtype(bits))
    plant = [0, (1 << bits) - 1] + [q - 1 for q in qs] + [q for q in qs]
    for i, v in enumerate(plant):
        x[(7 * i + 3) % size] = v
        x[size - 1 - (5 * i) % size] = v
    return x


def canonical_key(g, rng, bits, moduli, polys, n):
    """polys x N canonical words, polynomial i modulo moduli[i % len(moduli)]"""
    dt = g.np_dtype(bits)
    return np.concatenate([rng.integers(0, moduli[i % len(moduli)], size=n, dtype=np.uint64).astype(dt)
                           for i in range(polys)])


def elements_for(g, n_power, G):
    """rotation by +1 and -1, conjugation, the identity and one duplicate; further rotations beyond five"""
    base = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_rotation(-1, n_power),
            g.galois_element_for_conjugation(n_power), 1, g.galois_element_for_rotation(1, n_power)]
    return (base + [g.galois_element_for_rotation(s, n_power) for s in range(2, G)])[:G]


def composition(g, plan, st, a, c0, keys, elts, count, output_ntt):
    """rotate_hoisted's definition through the calls that existed before it; returns out T[G][2][count][L][N].
    a, c0, keys: device tensors.  c0 may hold any words: "added mod q_m" reads them modulo q_m, done here on the host
    with numpy's exact unsigned % before anything else (the transforms are only defined on residues)."""
    import torch
    bits, n_power, L, M, D = plan.bits, plan.n_power, plan.q_count, plan.mod_count, plan.digits
    n, G, poly = 1 << n_power, len(elts), st["poly"]
    a_rot = filled(bits, G * D * count * M * n)
    g.GPU_Automorphism_NTT(a, a_rot, elts, n_power, poly, D * count * M)
    a_rot = a_rot.view(G, -1)
    if c0 is not None:
        qs = np.array(st["moduli"][:L], dtype=g.np_dtype(bits))
        red = g.to_host(c0).reshape(count, L, n) % qs[None, :, None]
        c0_rot = filled(bits, G * count * L * n)
        g.GPU_Automorphism_NTT(g.to_device(red.reshape(-1)), c0_rot, elts, n_power, poly, count * L)
        if not output_ntt:
            cfg_i = g.ntt_rns_configuration(n_power=n_power, ntt_type=g.INVERSE, reduction_poly=poly,
                                            mod_inverse=st["d_ninv"])
            g.GPU_INTT_Inplace(c0_rot, st["inv"], st["mods"], cfg_i, G * count * L, L)
        c0_rot = c0_rot.view(G, count, L, n)
        qt = g.to_device(qs).view(1, L, 1)
    out = filled(bits, G * 2 * count * L * n).view(G, 2, count, L, n)
    scratch = torch.zeros(plan.scratch_bytes(count, 2), dtype=torch.uint8, device="cuda:0")
    for i in range(G):
        plan.switch_digits(a_rot[i], keys[i], out[i].view(-1), count, 2, output_ntt, scratch)
        if c0 is not None:
            s = out[i, 0] + c0_rot[i]  # both below q < 2^(W-2): 2 q - 2 < 2^(W-1), no wrap in the signed type
            out[i, 0] = torch.where(s >= qt, s - qt, s)
    torch.cuda.synchronize()
    return out.view(-1)
