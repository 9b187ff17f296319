"""KeySwitchPlan.lift_small / generate_keys / encrypt_symmetric on the GPU (include/gpuntt/rns/key_switch.cuh, "Key
material"): every output word against tests/keygen_exact.py on the widest primes, the `a` planes untouched, a hipGraph
replay, the launch sequence and every refusal before a launch; and the semantic check -- keys and ciphertexts made on the
device really multiply and rotate, at a ring (2^13) the Python-integer keys of the older tests could not reach."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hoisted_exact import transform
from hoisted_utils import any_words, device_words, filled, make_plan, ring
from innerprod_utils import from_words
from keygen_exact import EDGES, exact_encrypt, exact_generate_keys, exact_lift
from keygen_utils import planted_errors
from keyswitch_utils import centre, crt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 2, 2), (3, 2, 1), (4, 1, 4)]  # a ragged last digit; alpha = 1; one digit
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def setup(g, bits, n_power, L, K, alpha, **kw):
    full = ring(g, bits, n_power, M=8, widths="wide")
    M = L + K
    st = full.sub(list(range(M)))
    return full.cases[:M], st, make_plan(g, st, L, alpha, n_power, bits, **kw)


def scratch_of(nbytes):
    import torch
    return torch.zeros(max(256, nbytes), dtype=torch.uint8, device="cuda:0")


def small_device(x, offset=0):
    import torch
    t = torch.zeros(x.size + offset, dtype=torch.int32, device="cuda:0")
    t[offset:] = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to("cuda:0")
    return t[offset:]


def host(g, t, shape):
    return from_words(g.to_host(t), shape)


# --------------------------------------------------------------------------------------------------------- lift_small
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
def test_lift_small_every_word(g, bits, n_power):
    """the edge values INT32_MIN, -1, 0, INT32_MAX in every polynomial, both bases, with and without the transform, the
    operands aligned and one word off alignment"""
    import torch
    L, K, alpha, polys = 3, 2, 2, 3
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    n = 1 << n_power
    small = planted_errors(np.random.default_rng(n_power), (polys, n))
    assert all(v in small for v in EDGES)
    for full_base in (True, False):
        B = L + K if full_base else L
        for to_ntt in (False, True):
            want = exact_lift(cases[:B], small, to_ntt)
            for offset in (0, 1):
                d_small = small_device(small, offset)
                out = filled(bits, polys * B * n + 16, offset, GUARD)
                with g.launch_log() as log:
                    plan.lift_small(d_small, out, polys, full_base, to_ntt)
                torch.cuda.synchronize()
                assert log.kernels[0] == "lift_small" and log.kernels.count("lift_small") == 1
                assert (len(log.kernels) == 1) == (not to_ntt)
                assert np.array_equal(host(g, out[:polys * B * n], want.shape), want), (full_base, to_ntt, offset)
                assert (g.to_host(out[polys * B * n:]) == GUARD).all()
                assert np.array_equal(g.to_host(d_small, signed=True).reshape(small.shape), small)


# ------------------------------------------------------------------------------------------------------ generate_keys
def key_inputs(g, plan, st, rng, keys, offset=0):
    """s, s_from and the keys' `a` planes of any words; errors with the edges planted; component 0 at a guard value"""
    bits, n, M, D = plan.bits, 1 << plan.n_power, plan.mod_count, plan.digits
    qs = st["moduli"]
    s = device_words(g, any_words(g, rng, bits, M * n, qs), offset)
    s_from = device_words(g, any_words(g, rng, bits, keys * M * n, qs), offset)
    errors = planted_errors(rng, (keys, D, n))
    a = any_words(g, rng, bits, keys * D * M * n, qs).reshape(keys, D, M, n)
    dev = []
    for i in range(keys):
        k = filled(bits, D * 2 * M * n + 16, offset, GUARD)
        k[:D * 2 * M * n].view(D, 2, M, n)[:, 1] = g.to_device(a[i]).view(D, M, n)
        dev.append(k)
    return s, s_from, errors, a, dev


def check_keys(g, cases, plan, s, s_from, errors, a, dev):
    bits, n, M, D, L = plan.bits, 1 << plan.n_power, plan.mod_count, plan.digits, plan.q_count
    keys = len(dev)
    want = exact_generate_keys(cases, L, plan.alpha, host(g, s, (M, n)), host(g, s_from, (keys, M, n)), errors,
                               a.astype(object))
    for i, k in enumerate(dev):
        got = host(g, k[:D * 2 * M * n], (D, 2, M, n))
        assert np.array_equal(got[:, 0], want[i]), i
        assert np.array_equal(got[:, 1], a[i].astype(object)), i  # a is as it was
        assert (g.to_host(k[D * 2 * M * n:]) == GUARD).all(), i


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 12])
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_generate_keys_every_output_word(g, bits, n_power, L, K, alpha):
    import torch
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    rng = np.random.default_rng(100 * n_power + L)
    for keys in (1, 3):
        s, s_from, errors, a, dev = key_inputs(g, plan, st, rng, keys)
        plan.generate_keys(s, s_from, small_device(errors), [k[:-16] for k in dev],
                           scratch_of(plan.keygen_scratch_bytes(keys)))
        torch.cuda.synchronize()
        check_keys(g, cases, plan, s, s_from, errors, a, dev)


@pytest.mark.parametrize("bits", [64, 32])
def test_generate_keys_sixty_four_keys_and_off_alignment(g, bits):
    """64 keys in one call at n_power 5; then every operand one word off 16-byte alignment (the one-word loader)"""
    import torch
    n_power, L, K, alpha = 5, 5, 2, 2
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    for keys, offset in ((64, 0), (2, 1)):
        rng = np.random.default_rng(keys)
        s, s_from, errors, a, dev = key_inputs(g, plan, st, rng, keys, offset)
        with g.launch_log() as log:
            plan.generate_keys(s, s_from, small_device(errors, offset), [k[:-16] for k in dev],
                               scratch_of(plan.keygen_scratch_bytes(keys)))
        torch.cuda.synchronize()
        assert log.kernels[0] == "lift_small" and log.kernels[-1] == "keygen_combine"
        assert log.kernels.count("lift_small") == 1 and log.kernels.count("keygen_combine") == 1
        check_keys(g, cases, plan, s, s_from, errors, a, dev)


# -------------------------------------------------------------------------------------------------- encrypt_symmetric
def decrypt(g, cases, L, ct, s_ntt):
    """ct [2][L][N] and s_ntt [>= L][N] in NTT form (object words) -> c0 + c1 s as centred integers modulo Q"""
    qs = [c.q for c in cases[:L]]
    v = np.stack([(ct[0, m] + ct[1, m] * s_ntt[m]) % q for m, q in enumerate(qs)])
    Q = math.prod(qs)
    return centre(crt(transform(cases[:L], v, True), qs), Q), Q


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 12])
def test_encrypt_symmetric_every_word_and_it_decrypts(g, bits, n_power):
    """word for word against the model with `a` and the message of any words; then a real instance -- ternary s, small
    errors, a message lifted on the device -- decrypts to e + m exactly"""
    import torch
    L, K, alpha, count = 3, 2, 2, 3
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    M, n = L + K, 1 << n_power
    qs = st["moduli"]
    rng = np.random.default_rng(n_power + bits)
    s = device_words(g, any_words(g, rng, bits, M * n, qs))
    errors = planted_errors(rng, (count, n))
    for with_message in (True, False):
        message = device_words(g, any_words(g, rng, bits, count * L * n, qs[:L])) if with_message else None
        a = any_words(g, rng, bits, count * L * n, qs[:L])
        out = filled(bits, 2 * count * L * n + 16, 0, GUARD)
        out[count * L * n:2 * count * L * n] = g.to_device(a)
        with g.launch_log() as log:
            plan.encrypt_symmetric(s, small_device(errors), message, out[:-16], count,
                                   scratch_of(plan.encrypt_scratch_bytes(count)))
        torch.cuda.synchronize()
        assert log.kernels[0] == "lift_small" and log.kernels[-1] == "keygen_combine"
        assert log.kernels.count("lift_small") == 1 and log.kernels.count("keygen_combine") == 1
        want = exact_encrypt(cases, L, host(g, s, (M, n)), errors,
                             host(g, message, (count, L, n)) if with_message else None,
                             a.astype(object).reshape(count, L, n))
        got = host(g, out[:2 * count * L * n], (2, count, L, n))
        assert np.array_equal(got[0], want), with_message
        assert np.array_equal(got[1].reshape(-1), a.astype(object)) and (g.to_host(out[-16:]) == GUARD).all()

    # a real instance, everything made on the device
    s_small = filled(32, n)
    g.sample_small(s_small, 1, n_power, g.TERNARY, 41)
    s_ntt = filled(bits, M * n)
    plan.lift_small(s_small, s_ntt, 1, True, True)
    e = planted_errors(rng, (count, n), bound=20)
    m = rng.integers(-1000, 1001, size=(count, n), dtype=np.int64).astype(np.int32)
    msg = filled(bits, count * L * n)
    plan.lift_small(small_device(m), msg, count, False, True)
    ct = filled(bits, 2 * count * L * n)
    g.sample_uniform(ct[count * L * n:], qs[:L], n_power, count, 42)
    plan.encrypt_symmetric(s_ntt, small_device(e), msg, ct, count, scratch_of(plan.encrypt_scratch_bytes(count)))
    torch.cuda.synchronize()
    got, sh = host(g, ct, (2, count, L, n)), host(g, s_ntt, (M, n))
    for r in range(count):
        value, _ = decrypt(g, cases, L, got[:, r], sh)
        assert [int(v) for v in value] == [int(x) + int(y) for x, y in zip(e[r], m[r])], r


# ------------------------------------------------------------------------------------------- graphs, launches, refusals
@pytest.mark.parametrize("bits", [64, 32])
def test_captured_into_a_graph_and_replayed_with_new_data(g, bits):
    import torch
    n_power, L, K, alpha, keys, count = 9, 3, 2, 2, 2, 2
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    M, n, D = L + K, 1 << n_power, plan.digits
    s, s_from, errors, a, dev = key_inputs(g, plan, st, np.random.default_rng(0), keys)
    d_err = small_device(errors)
    d_err2 = small_device(errors[0, :count])
    ct = filled(bits, 2 * count * L * n, 0, 7)
    ks, es = scratch_of(plan.keygen_scratch_bytes(keys)), scratch_of(plan.encrypt_scratch_bytes(count))

    def both(stream):
        plan.generate_keys(s, s_from, d_err, [k[:-16] for k in dev], ks, stream=stream)
        plan.encrypt_symmetric(s, d_err2, None, ct, count, es, stream=stream)
    st_ = torch.cuda.Stream()
    st_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st_):  # eager warm-up on the capture stream
        both(st_)
    st_.synchronize()
    allocs = g.alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st_):
        both(st_)
    for seed in (1, 2):
        ns, nf, nerr, na, _ = key_inputs(g, plan, st, np.random.default_rng(seed), keys)
        s.copy_(ns), s_from.copy_(nf), d_err.copy_(small_device(nerr)), d_err2.copy_(small_device(nerr[1, :count]))
        for i, k in enumerate(dev):
            k[:D * 2 * M * n].view(D, 2, M, n)[:, 1] = g.to_device(na[i]).view(D, M, n)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check_keys(g, cases, plan, s, s_from, nerr, na, dev)
        got = host(g, ct, (2, count, L, n))
        want = exact_encrypt(cases, L, host(g, s, (M, n)), nerr[1, :count], None, got[1])
        assert np.array_equal(got[0], want), seed
    assert g.alloc_count() == allocs


def test_launches_memory_zero_counts_and_refusals(g):
    import torch
    bits, n_power, L, K, alpha = 64, 6, 5, 2, 2
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    M, n, D = L + K, 1 << n_power, plan.digits
    rng = np.random.default_rng(3)
    lengths = {}
    for keys in (1, 3):
        s, s_from, errors, a, dev = key_inputs(g, plan, st, rng, keys)
        d_err, scratch = small_device(errors), scratch_of(plan.keygen_scratch_bytes(keys))
        torch.cuda.synchronize()
        held, allocs = torch.cuda.memory_allocated(), g.alloc_count()
        with g.launch_log() as log:
            plan.generate_keys(s, s_from, d_err, [k[:-16] for k in dev], scratch)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == held and g.alloc_count() == allocs
        lengths[keys] = len(log.kernels)
    assert lengths[1] == lengths[3]  # no step's launch count grows with the keys
    assert plan.keygen_scratch_bytes(3) == -(-3 * D * M * n * 8 // 256) * 256 and plan.keygen_scratch_bytes(0) == 0

    keys = 2
    s, s_from, errors, a, dev = key_inputs(g, plan, st, rng, keys)
    ks = [k[:-16] for k in dev]
    d_err = small_device(errors)
    sbytes = plan.keygen_scratch_bytes(keys)
    big = scratch_of(sbytes + 256)
    scratch, words64 = big[:sbytes], big[:sbytes].view(torch.int64)
    count = 2
    ct, msg = filled(bits, 2 * count * L * n), filled(bits, count * L * n)
    e1, es = small_device(errors[0, :count]), scratch_of(plan.encrypt_scratch_bytes(count))
    small, lifted = small_device(errors[0]), filled(bits, D * M * n)
    with g.launch_log() as log:
        plan.generate_keys(s, s_from, d_err, [], scratch)
        plan.encrypt_symmetric(s, e1, msg, ct, 0, es)
        plan.lift_small(small, lifted, 0, True, True)
    assert log.kernels == []
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    wider = make_plan(g, st, L, alpha, n_power, bits, key_mod_count=M + 1, key_limbs=list(range(M)))
    permuted = make_plan(g, st, L, alpha, n_power, bits, key_limbs=[1, 0] + list(range(2, M)))
    gen, enc, lift = plan.generate_keys, plan.encrypt_symmetric, plan.lift_small
    key_words = D * 2 * M * n
    pair = filled(bits, key_words + 8)
    refused = [lambda: gen(None, s_from, d_err, ks, scratch),
               lambda: gen(s, None, d_err, ks, scratch),
               lambda: gen(s, s_from, None, ks, scratch),
               lambda: gen(s, s_from, d_err, [ks[0], None], scratch),
               lambda: gen(s, s_from, d_err, ks, None),
               lambda: gen(s, s_from, d_err, ks * 33, scratch),                         # 66 keys
               lambda: gen(s, s_from, d_err, ks, big[8:8 + sbytes]),                    # not 256-byte aligned
               lambda: gen(s, s_from, d_err, ks, scratch[:-256]),                       # too small
               lambda: gen(s[1:], s_from, d_err, ks, scratch),
               lambda: gen(s, s_from[1:], d_err, ks, scratch),
               lambda: gen(s, s_from, d_err[1:], ks, scratch),
               lambda: gen(s, s_from, d_err, [ks[0], ks[1][1:]], scratch),
               lambda: gen(s, s_from, d_err.to(torch.int64), ks, scratch),
               lambda: gen(s, s_from, d_err, [ks[0], ks[0]], scratch),                  # the same key twice
               lambda: gen(s, s_from, d_err, [pair[:key_words], pair[8:]], scratch),    # two keys that overlap
               lambda: gen(ks[0][:M * n], s_from, d_err, ks, scratch),                  # s inside a key
               lambda: gen(s, ks[1][:keys * M * n], d_err, ks, scratch),                # s_from inside a key
               lambda: gen(words64[:M * n], s_from, d_err, ks, scratch),                # the scratch over s
               lambda: gen(s, words64[:keys * M * n], d_err, ks, scratch),
               lambda: gen(s, s_from, big[:sbytes].view(torch.int32)[:keys * D * n], ks, scratch),
               lambda: gen(s, s_from, d_err, [ks[0], words64[:key_words]], scratch),
               lambda: bare.generate_keys(s, s_from, d_err, ks, scratch),               # no transforms
               lambda: wider.generate_keys(s, s_from, d_err, ks, scratch),              # key_mod_count != M
               lambda: permuted.generate_keys(s, s_from, d_err, ks, scratch),           # key_limbs not the identity
               lambda: enc(None, e1, msg, ct, count, es),
               lambda: enc(s, None, msg, ct, count, es),
               lambda: enc(s, e1, msg, None, count, es),
               lambda: enc(s, e1, msg, ct, count, None),
               lambda: enc(s, e1, msg, ct, -1, es),
               lambda: enc(s, e1, msg, ct[1:], count, es),
               lambda: enc(s, e1, msg[1:], ct, count, es),
               lambda: enc(s, e1[1:], msg, ct, count, es),
               lambda: enc(s, e1, ct[:count * L * n], ct, count, es),                   # the message inside out
               lambda: enc(ct[:M * n], e1, msg, ct, count, es),                         # s inside out
               lambda: enc(s, e1, msg, words64[:2 * count * L * n], count, big[:plan.encrypt_scratch_bytes(count)]),
               lambda: enc(s, e1, msg, ct, count, big[8:8 + plan.encrypt_scratch_bytes(count)]),
               lambda: bare.encrypt_symmetric(s, e1, msg, ct, count, es),
               lambda: lift(None, lifted, D, True, False),
               lambda: lift(small, None, D, True, False),
               lambda: lift(small, lifted, -1, True, False),
               lambda: lift(small, lifted[1:], D, True, False),
               lambda: lift(small[1:], lifted, D, True, False),
               lambda: lift(small, lifted.view(torch.int32)[:D * n], D, True, False),   # not the plan's word type
               lambda: lift(lifted.view(torch.int32)[:D * n], lifted, D, True, False),  # the input inside the output
               lambda: bare.lift_small(small, lifted, D, True, True)]                   # to_ntt without transforms
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises((ValueError, RuntimeError)):
                f()
        assert log.kernels == [], i
    with g.launch_log() as log:
        bare.lift_small(small, lifted, D, True, False)  # the lift alone needs no transforms
    assert log.kernels == ["lift_small"]
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------- it really is key material
def sigma(x, k):
    """a(X) -> a(X^k) in Z[X] / (X^N + 1), vectorised"""
    n = len(x)
    e = (np.arange(n, dtype=np.int64) * int(k)) % (2 * n)
    out = np.zeros(n, dtype=object)
    out[e % n] = np.where(e < n, 1, -1).astype(object) * x
    return out


@pytest.mark.parametrize("bits,n_power", [(64, 5), (32, 5), (64, 13)])
def test_device_made_keys_and_ciphertexts_really_multiply_and_rotate(g, bits, n_power):
    """Everything on the device: a ternary secret (sample_small, lift_small), s^2 by operator_gpu and sigma_k(s) by
    GPU_Automorphism_NTT, three switching keys in ONE generate_keys call with all errors zero (a relinearization key,
    rotation by 1, conjugation; `a` from sample_uniform), two encryptions of small messages.  multiply_relinearize, apply
    and rotate_hoisted on them decrypt -- in the NTT domain, so that 2^13 is within reach -- to the product, to c1 s^2
    and to sigma_k(m) within the bound the existing tests derive for a noiseless key: the accumulators satisfy
    A_0 + A_1 s = P X (mod P Q) exactly, each of the two ModDowns is off from A_c / P by at most 1/2 (and the rounding
    band), and (1, s) weighs them by 1 + h, h = |s|_1: at most (1 + h) / 2 + 1 per ModDown'd component pair."""
    import torch
    L, K, alpha = 3, 2, 2
    cases, st, plan = setup(g, bits, n_power, L, K, alpha)
    M, n, D = L + K, 1 << n_power, plan.digits
    full, qs, poly = st["moduli"], st["moduli"][:L], st["poly"]
    mods = [c.prm.modulus for c in cases]
    elts = [g.galois_element_for_rotation(1, n_power), g.galois_element_for_conjugation(n_power)]

    s_small = filled(32, n)
    g.sample_small(s_small, 1, n_power, g.TERNARY, 2024, 0)
    s_ntt = filled(bits, M * n)
    plan.lift_small(s_small, s_ntt, 1, True, True)
    s_from = filled(bits, 3 * M * n)
    for m in range(M):  # s^2, limb by limb
        s_from[m * n:(m + 1) * n] = g.operator_gpu(2, s_ntt[m * n:(m + 1) * n], s_ntt[m * n:(m + 1) * n], mods[m])
    g.GPU_Automorphism_NTT(s_ntt, s_from[M * n:], elts, n_power, poly, M)
    keys = [filled(bits, D * 2 * M * n) for _ in range(3)]
    for i, k in enumerate(keys):
        g.sample_uniform(k[M * n:], full, n_power, D, 7, i, stack_stride_words=2 * M * n)
    zeros = torch.zeros(3 * D * n, dtype=torch.int32, device="cuda:0")
    plan.generate_keys(s_ntt, s_from, zeros, keys, scratch_of(plan.keygen_scratch_bytes(3)))

    rng = np.random.default_rng(n_power)
    msgs = rng.integers(-1000, 1001, size=(2, n), dtype=np.int64).astype(np.int32)
    cts = []
    for i in range(2):
        msg, ct = filled(bits, L * n), filled(bits, 2 * L * n)
        plan.lift_small(small_device(msgs[i]), msg, 1, False, True)
        g.sample_uniform(ct[L * n:], qs, n_power, 1, 8, i)
        plan.encrypt_symmetric(s_ntt, zeros[:n], msg, ct, 1, scratch_of(plan.encrypt_scratch_bytes(1)))
        cts.append(ct)
    torch.cuda.synchronize()

    sh = host(g, s_ntt, (M, n))
    s_int = np.array([int(v) for v in g.to_host(s_small, signed=True)], dtype=object)
    h = int(sum(abs(v) for v in s_int))
    bound = (1 + h) / 2 + 1
    m_int = [np.array([int(v) for v in msgs[i]], dtype=object) for i in range(2)]
    for i in range(2):  # the inputs themselves are exact
        value, Q = decrypt(g, cases, L, host(g, cts[i], (2, L, n)), sh)
        assert all(int(a) == int(b) for a, b in zip(value, m_int[i]))

    def ring_product(x_ntt, y_ntt):
        """[L][N] x [L][N] in NTT form -> the product modulo Q, centred"""
        v = np.stack([(x_ntt[m] * y_ntt[m]) % q for m, q in enumerate(qs)])
        return centre(crt(transform(cases[:L], v, True), qs), Q)

    def error(value, want):
        return max(abs(int(v)) for v in centre((value - want) % Q, Q))

    scratch = scratch_of(plan.scratch_bytes(1, 2))
    m_ntt = [exact_lift(cases[:L], msgs[i:i + 1], True)[0] for i in range(2)]
    # ct x ct under the relinearization key
    out = filled(bits, 2 * L * n)
    plan.multiply_relinearize(cts[0], cts[1], keys[0], out, 1, True, scratch)
    torch.cuda.synchronize()
    value, _ = decrypt(g, cases, L, host(g, out, (2, L, n)), sh)
    errs = [error(value, ring_product(m_ntt[0], m_ntt[1]))]
    # apply: c1 switched from s^2 to s
    c1 = host(g, cts[0], (2, L, n))[1]
    plan.apply(cts[0][L * n:], keys[0], out, 1, 2, True, True, scratch)
    torch.cuda.synchronize()
    value, _ = decrypt(g, cases, L, host(g, out, (2, L, n)), sh)
    s2 = np.stack([(sh[m] * sh[m]) % q for m, q in enumerate(qs)])
    errs.append(error(value, ring_product(c1, s2)))
    # two hoisted rotations of one decomposition
    a = filled(bits, D * M * n)
    plan.decompose(cts[0][L * n:], a, 1, True, scratch)
    rot = filled(bits, 2 * 2 * L * n)
    plan.rotate_hoisted(a, cts[0][:L * n], keys[1:], elts, rot, 1, True, scratch_of(plan.hoisted_scratch_bytes(1, 2)))
    torch.cuda.synchronize()
    got = host(g, rot, (2, 2, L, n))
    for i, k in enumerate(elts):
        value, _ = decrypt(g, cases, L, got[i], sh)
        errs.append(error(value, sigma(m_int[0], k)))
    print("h = %d, bound %.1f, errors (product, apply, rotation, conjugation): %s" % (h, bound, errs))
    assert max(errs) <= bound, (errs, bound)


def test_cpp_caller_of_the_public_headers(g):
    """tests/cpp/example_keygen_rotate.cpp, compiled here against include/ and libgpuntt.so: the secret, a rotation key and
    a ciphertext made on the device through the C++ interface, rotate_hoisted, and the host decrypts; it prints its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_keygen_rotate")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_keygen_rotate.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        for args in (("10",), ("8", "u32")):
            r = subprocess.run(["timeout", "-k", "10", "120", exe, *args], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
