"""Hybrid key switching without a GPU (include/gpuntt/rns/key_switch.cuh): the constants a plan uploads
(gpuntt_keyswitch_constants_*) against the per-digit constants of BaseConvPlan and Python integers, the host references
(gpuntt_keyswitch_reference_mod_up_* / _mod_down_*) against the header's formulas restated in Python integers, and
everything the host refuses before a device is touched.  The references run the argument checks of the calls
themselves, so the refusals are those of mod_up / mod_down."""
import ctypes

import numpy as np
import pytest

from innerprod_utils import from_words, moduli, words
from keyswitch_utils import SHAPES, partition, planted_input, ref_mod_down, ref_mod_up


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def bases(bits, L, K):
    ms = moduli(bits, L + K)
    return ms[:L], ms[L:L + K]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_constants_are_the_per_digit_base_conversion_constants(g, bits, L, K, alpha):
    qs, ps = bases(bits, L, K)
    full, M, W = qs + ps, L + K, bits
    c = g.keyswitch_constants(qs, ps, alpha, bits)
    parts = partition(L, alpha)
    assert c["up_q_mod"].shape == (len(parts), M) and c["up_matrix"].shape == (L, M)
    for d, S in enumerate(parts):
        S = list(S)
        rest = [m for m in range(M) if m not in S]
        b = g.baseconv_constants([qs[i] for i in S], [full[m] for m in rest], bits)
        for name in ("qhat_inv", "qhat_inv_shoup", "recip", "bit_length"):
            assert np.array_equal(c["up_" + name][S], b[name]), (d, name)
        assert np.array_equal(c["up_matrix"][S][:, rest], b["matrix"]), d
        assert np.array_equal(c["up_q_mod"][d][rest], b["q_mod_p"]), d
        assert not c["up_matrix"][S][:, S].any() and not c["up_q_mod"][d][S].any()
    b = g.baseconv_constants(ps, qs, bits)
    for mine, theirs in (("down_qhat_inv", "qhat_inv"), ("down_qhat_inv_shoup", "qhat_inv_shoup"),
                         ("down_matrix", "matrix"), ("down_p_mod_q", "q_mod_p"), ("down_p_inv_mod_q", "q_inv_mod_p"),
                         ("down_recip", "recip"), ("down_bit_length", "bit_length")):
        assert np.array_equal(c[mine], b[theirs]), mine
    for m, q in enumerate(full):
        t1, t2 = (1 << W) % q, (1 << 2 * W) % q
        assert int(c["pow_w"][m]) == t1 and int(c["pow_w_shoup"][m]) == (t1 << W) // q
        assert int(c["pow_2w"][m]) == t2 and int(c["pow_2w_shoup"][m]) == (t2 << W) // q
        assert int(c["one_shoup"][m]) == (1 << W) // q


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("n_power", [1, 5])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_references_against_python_integers(g, bits, L, K, alpha, n_power, count):
    qs, ps = bases(bits, L, K)
    M, n, D = L + K, 1 << n_power, len(partition(L, alpha))
    rng = np.random.default_rng(1000 * L + 10 * K + alpha + n_power + bits)
    x = planted_input(rng, bits, qs, (count, L, n))
    wx = words(g, x, bits)
    keep = wx.copy()
    for mode in (g.APPROXIMATE, g.CENTRED):
        a = np.full(D * count * M * n, (1 << bits) - 1, dtype=g.np_dtype(bits))
        assert g.keyswitch_reference_mod_up(qs, ps, alpha, wx, a, n_power, count, mode, bits) is a
        assert np.array_equal(wx, keep)
        want = ref_mod_up(qs, ps, alpha, x, bits, mode == g.CENTRED)
        assert np.array_equal(from_words(a, want.shape), want), mode
    stacks = count
    xs = planted_input(rng, bits, qs + ps, (stacks, M, n))
    out = np.full(stacks * L * n, (1 << bits) - 1, dtype=g.np_dtype(bits))
    g.keyswitch_reference_mod_down(qs, ps, words(g, xs, bits), out, n_power, stacks, bits)
    want = ref_mod_down(qs, ps, xs, bits)
    assert np.array_equal(from_words(out, want.shape), want)


def test_mod_down_rounds_the_integer_outside_the_band(g):
    """the residues of one integer C in [0, PQ): the result is round(C / P) mod q_j (ties and the band aside)"""
    import math
    bits, n_power = 64, 3
    qs, ps = bases(bits, 3, 2)
    P, Q = math.prod(ps), math.prod(qs)
    rng = np.random.default_rng(5)
    C = [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % (P * Q)
         for _ in range(8)]
    x = np.array([[c % m for c in C] for m in qs + ps], dtype=object).reshape(1, 5, 8)
    out = np.zeros(3 * 8, dtype=np.uint64)
    g.keyswitch_reference_mod_down(qs, ps, words(g, x, bits), out, n_power, 1, bits)
    got = from_words(out, (3, 8))
    for j, q in enumerate(qs):
        assert [int(v) for v in got[j]] == [((2 * c + P) // (2 * P)) % q for c in C]


def test_everything_the_host_refuses(g):
    bits, n_power, count = 64, 3, 2
    qs, ps = bases(bits, 5, 2)
    L, K, M, alpha, n = 5, 2, 7, 2, 8
    x = np.zeros(count * L * n, dtype=np.uint64)
    a = np.zeros(3 * count * M * n, dtype=np.uint64)

    def up(qs=qs, ps=ps, alpha=alpha, x=x, a=a, n_power=n_power, count=count, mode=g.CENTRED, bits=bits):
        g.keyswitch_reference_mod_up(qs, ps, alpha, x, a, n_power, count, mode, bits)

    buf = np.zeros(x.size + a.size, dtype=np.uint64)
    refused_up = [
        dict(n_power=0), dict(n_power=29), dict(alpha=0), dict(alpha=-1), dict(count=-1), dict(mode=2), dict(x=None),
        dict(a=None), dict(qs=[]), dict(ps=[]), dict(qs=moduli(64, 64), ps=moduli(64, 65)[64:]),  # M = 65
        dict(qs=qs[:4] + [qs[0]]), dict(ps=[ps[0], qs[1]]), dict(ps=[ps[0] * 3, 15]),               # not coprime
        dict(qs=qs[:4] + [g.Modulus(qs[4], 63, 1, 64)]), dict(qs=qs[:4] + [1]),                     # "Invalid modulus!"
        dict(x=buf[:x.size], a=buf[x.size - 1:]), dict(x=buf[a.size - 1:], a=buf[:a.size]),         # overlap
        dict(x=x[1:]), dict(a=a[1:]), dict(x=x.astype(np.uint32)),                                  # short, wrong type
    ]
    for kw in refused_up:
        with pytest.raises(ValueError):
            up(**kw)
    up()
    with pytest.raises(ValueError, match="Invalid modulus!"):
        up(qs=qs[:4] + [g.Modulus(qs[4], 63, 1, 64)])
    with pytest.raises(ValueError, match="Invalid n_power range!"):
        up(n_power=29)

    xs = np.zeros(count * M * n, dtype=np.uint64)
    out = np.zeros(count * L * n, dtype=np.uint64)

    def down(qs=qs, ps=ps, x=xs, out=out, n_power=n_power, stacks=count):
        g.keyswitch_reference_mod_down(qs, ps, x, out, n_power, stacks, bits)

    for kw in [dict(n_power=0), dict(n_power=29), dict(stacks=-1), dict(x=None), dict(out=None), dict(qs=[]),
               dict(ps=[]), dict(ps=[qs[0]]), dict(x=xs[1:]), dict(out=out[1:]), dict(x=xs, out=xs),
               dict(x=buf[:xs.size], out=buf[xs.size - 1:])]:
        with pytest.raises(ValueError):
            down(**kw)
    down()
    # count = 0 and stacks = 0 do nothing
    a[:] = 7
    up(count=0)
    assert (a == 7).all()
    for args in ((0, 1, 1, 3), (1, 0, 1, 3), (60, 5, 1, 3), (3, 1, 0, 3), (3, 1, 1, 0), (3, 1, 1, 29)):
        with pytest.raises(ValueError):
            g.KeySwitchPlan.workspace_bytes(*args)
    with pytest.raises(ValueError):
        g.keyswitch_constants(qs, [qs[0]], 2)
    assert g.KeySwitchPlan.workspace_bytes(63, 1, 1, 28) > 0


def test_everything_the_constructor_and_the_scratch_size_refuse(g):
    """gpuntt_keyswitch_plan_create_* through its return codes: every refusal below is thrown before the first HIP
    call, so no device is needed (a table pointer that is never dereferenced stands for a device table)"""
    bits, L, K, alpha, n_power = 64, 4, 2, 2, 5
    qs, ps = bases(bits, L, K)
    M = L + K
    lib = g.load_library()
    table = ctypes.c_void_p(0x1000)
    ninv = (ctypes.c_uint64 * M)(*([1] * M))

    def create(qs=qs, ps=ps, alpha=alpha, n_power=n_power, fwd=None, inv=None, ninv=None, poly=g.X_N_plus, km=M,
               limbs=None, handle=True):
        marr = lambda ms: (g._M64 * max(1, len(ms)))(*[g.Modulus(int(m), bits=64).c() for m in ms])
        h = ctypes.c_void_p()
        arr = None if limbs is None else (ctypes.c_int * len(limbs))(*limbs)
        rc = lib.gpuntt_keyswitch_plan_create_u64(ctypes.byref(h) if handle else None, marr(qs), len(qs), marr(ps),
                                                  len(ps), alpha, n_power, fwd, inv, ninv, poly, 1, km, arr, None, None)
        assert not h.value
        return rc, lib.gpuntt_last_error().decode()

    refused = [
        dict(km=M - 1), dict(km=257), dict(km=0),                                        # key_mod_count outside [M, 256]
        dict(limbs=[0, 1, 2, 3, 4, M]), dict(limbs=[0, 1, 2, 3, 4, -1]), dict(km=8, limbs=[0, 1, 2, 3, 6, 8]),
        dict(fwd=table), dict(inv=table), dict(fwd=table, inv=table),                    # tables without the rest
        dict(fwd=table, ninv=ninv), dict(inv=table, ninv=ninv),
        dict(alpha=0), dict(n_power=0), dict(n_power=29), dict(qs=[]), dict(ps=[]), dict(poly=2),
        dict(qs=moduli(64, 64), ps=moduli(64, 65)[64:]), dict(ps=[ps[0], qs[1]]), dict(qs=qs[:3] + [qs[0]]),
        dict(handle=False),
    ]
    for kw in refused:
        rc, msg = create(**kw)
        assert rc == -1 and msg, (kw, rc, msg)  # GPUNTT_ERR_INVALID_ARGUMENT
    assert create(km=M - 1)[1] == "Invalid key_mod_count!" and create(limbs=[0, 1, 2, 3, 4, M])[1] == "Invalid key_limbs!"
    assert create(n_power=29)[1] == "Invalid n_power range!"

    # a [D][count][M][N], the coefficient form of the input [count][L][N], the accumulators [C][count][M][N]; D = 2
    assert g.keyswitch_scratch_bytes(L, K, alpha, n_power, 3, 2) == (2 * 3 * M + 3 * L + 2 * 3 * M) * 32 * 8
    assert g.keyswitch_scratch_bytes(L, K, alpha, n_power, 0, 1) == 0
    for args in ((L, K, alpha, n_power, -1, 1), (L, K, alpha, n_power, 1, 0), (L, K, alpha, n_power, 1, 5),
                 (0, K, alpha, n_power, 1, 1), (L, 0, alpha, n_power, 1, 1), (L, K, 0, n_power, 1, 1),
                 (L, K, alpha, 0, 1, 1), (L, K, alpha, 29, 1, 1), (63, 2, 1, n_power, 1, 1)):
        with pytest.raises(ValueError):
            g.keyswitch_scratch_bytes(*args)
