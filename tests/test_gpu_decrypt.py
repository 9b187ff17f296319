"""KeySwitchPlan.phase / encrypt_public (include/gpuntt/rns/key_switch.cuh, "Decryption and public-key encryption") and
BfvMultiplyPlan.scale_message / decode / decrypt (include/gpuntt/rns/bfv_multiply.cuh, "Reading a result back") on the
GPU: every output word against tests/decrypt_exact.py, the launch sequence, a hipGraph replay, every refusal before a
launch, and the loop closed on device-made material -- encode, encrypt under a public key, multiply, decrypt, with the
noise budget before and after."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bfv_utils import bfv_scratch
from bfv_utils import make_plan as make_bfv_plan
from decrypt_exact import (exact_decode, exact_encrypt_public, exact_phase, exact_scale_message, noise_max, true_round)
from decrypt_utils import fresh_x, half_edges, random_x, residues, top_plain, usable
from hoisted_exact import transform
from hoisted_utils import any_words, device_words, filled, make_plan, ring
from innerprod_utils import from_words
from keygen_utils import planted_errors
from keyswitch_utils import crt
from relin3_utils import bases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
NARROW = (30, 29, 28, 27)  # the prime widths of the closed loop, for both word widths


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


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


def object_words(g, x, bits, offset=0):
    """an object array of words -> a device tensor"""
    return device_words(g, np.ascontiguousarray(x.astype(np.uint64).astype(g.np_dtype(bits)).reshape(-1)), offset)


# --------------------------------------------------------------------------------------------------------------- phase
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
@pytest.mark.parametrize("L,K,alpha", [(1, 1, 1), (3, 2, 2)])
def test_phase_every_word(g, bits, n_power, L, K, alpha):
    """components 2 and 3, both input and both output forms, the operands aligned and one word off alignment, on the
    widest primes; guard words after out, the inputs untouched, exactly one decrypt_phase besides the transforms; and out
    exactly ct in NTT form"""
    import torch
    full = ring(g, bits, n_power, M=8, widths="wide")
    st = full.sub(list(range(L + K)))
    cases, plan = full.cases[:L], make_plan(g, st, L, alpha, n_power, bits)
    M, n, count = L + K, 1 << n_power, 3
    qs = st["moduli"][:L]
    rng = np.random.default_rng(bits + n_power + L)
    s_w = any_words(g, rng, bits, M * n, st["moduli"])
    s_h = from_words(s_w, (M, n))
    for components in (2, 3):
        words = components * count * L * n
        ct_any = any_words(g, rng, bits, words, qs)
        ct_res = (from_words(ct_any, (components, count, L, n)) %
                  np.array(qs, dtype=object)[None, None, :, None])  # canonical: what a transform takes
        for input_ntt in (True, False):
            ct_h = from_words(ct_any, (components, count, L, n)) if input_ntt else ct_res
            for output_ntt in (True, False):
                want = exact_phase(cases, ct_h, s_h, input_ntt, output_ntt)
                for offset in (0, 1):
                    ct, s = object_words(g, ct_h, bits, offset), device_words(g, s_w, offset)
                    out = filled(bits, count * L * n + 16, offset, GUARD)
                    scratch = scratch_of(plan.phase_scratch_bytes(count, components, input_ntt))
                    with g.launch_log() as log:
                        plan.phase(ct, s, out[:-16], count, components, input_ntt, output_ntt,
                                   None if input_ntt else scratch)
                    torch.cuda.synchronize()
                    assert log.kernels.count("decrypt_phase") == 1
                    assert (len(log.kernels) == 1) == (input_ntt and output_ntt), log.kernels
                    if input_ntt:
                        assert log.kernels[0] == "decrypt_phase"
                    if output_ntt:
                        assert log.kernels[-1] == "decrypt_phase"
                    key = (components, input_ntt, output_ntt, offset)
                    assert np.array_equal(host(g, out[:count * L * n], want.shape), want), key
                    assert (g.to_host(out[count * L * n:]) == GUARD).all(), key
                    assert np.array_equal(host(g, ct, ct_h.shape), ct_h) and np.array_equal(g.to_host(s), s_w), key
        # out exactly ct, NTT form in: component 0 is overwritten, the others stay
        ct_h = from_words(ct_any, (components, count, L, n))
        ct = object_words(g, ct_h, bits)
        plan.phase(ct, device_words(g, s_w), ct, count, components, True, True)
        torch.cuda.synchronize()
        got = host(g, ct, ct_h.shape)
        assert np.array_equal(got[0], exact_phase(cases, ct_h, s_h, True, True)) and np.array_equal(got[1:], ct_h[1:])
    assert plan.phase_scratch_bytes(count, 3, True) == 0
    assert plan.phase_scratch_bytes(count, 3, False) == -(-3 * count * L * n * (bits // 8) // 256) * 256


# ------------------------------------------------------------------------------------------- scale_message and decode
def bfv_for(g, bits, n_power, L, t, widths):
    """the ring's first L primes and the smallest auxiliary base behind them"""
    full, st_b, st_p, _ = bases(g, bits, n_power, L, t, widths=widths)
    return full, st_b, st_p, make_bfv_plan(g, st_b, L, t, n_power, bits)


def vector_round(X, Q, t):
    """round-half-up(t X / Q) mod t over an object array: true_round, vectorised"""
    return ((2 * t * X + Q) // (2 * Q)) % t


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
@pytest.mark.parametrize("L", [1, 3])
def test_scale_message_and_decode_every_word(g, bits, n_power, L):
    """every prime of the top width, so that the largest t sits just below 2^(W-2).  decode on three stacks: any words
    with x = 0 and x = Q - 1, the planted half-edges, a full-width random batch; then fresh ciphertext phases with the
    largest noise planted in another column tile per stack (the first column, the middle, the last): messages and
    noise_max equal the model everywhere, the true rounding outside the model's mask"""
    import torch
    n, W = 1 << n_power, bits
    probe = ring(g, bits, n_power, M=2 * L + 6, widths=(bits - 2,))
    qs = probe.moduli[:L]
    Q = math.prod(qs)
    top = top_plain(qs, bits)
    assert top > (1 << (bits - 2)) - (1 << (bits - 8)) and usable(top, qs, bits)
    for t in (2, 257, 65537, top):
        _, st_b, _, plan = bfv_for(g, bits, n_power, L, t, (bits - 2,))
        assert st_b["moduli"][:L] == qs
        rng = np.random.default_rng(bits + n_power + L + t % 1000)
        # scale_message: any words, the edges of t planted; both forms; aligned and one word off
        msg_w = any_words(g, rng, bits, 3 * n, [t, t + 1, 1])
        want = exact_scale_message(qs, t, from_words(msg_w, (3, n)))
        for to_ntt in (False, True):
            w = transform(probe.cases[:L], want, False) if to_ntt else want
            for offset in (0, 1):
                out = filled(bits, 3 * L * n + 16, offset, GUARD)
                with g.launch_log() as log:
                    plan.scale_message(device_words(g, msg_w, offset), out[:-16], 3, to_ntt)
                torch.cuda.synchronize()
                assert log.kernels[0] == "bfv_scale_message" and log.kernels.count("bfv_scale_message") == 1
                assert (len(log.kernels) == 1) == (not to_ntt)
                assert np.array_equal(host(g, out[:3 * L * n], w.shape), w), (t, to_ntt, offset)
                assert (g.to_host(out[3 * L * n:]) == GUARD).all()

        # decode, the variety batch
        anyw = from_words(any_words(g, rng, bits, L * n, qs), (L, n))
        anyw[:, 0] = 0
        anyw[:, n - 1] = np.array([q - 1 for q in qs], dtype=object)  # x = Q - 1
        x = np.stack([anyw, residues(half_edges(rng, Q, t, n), qs), residues(random_x(rng, Q, n), qs)])
        # the leak batch: small noise everywhere, one large one per stack in its own column tile
        fresh, _ = fresh_x(rng, Q, t, 3 * n, bound=5)
        big = Q // (8 * t)
        for stk, col in enumerate((0, n // 2, n - 1)):
            fresh[stk * n + col] = (fresh[stk * n + col] + (stk + 1) * big // 4) % Q
        y = np.stack([residues(fresh[k * n:(k + 1) * n], qs) for k in range(3)])
        for batch, name in ((x, "variety"), (y, "leak")):
            m_want, n_want, band = exact_decode(qs, t, batch, W)
            X = np.stack([crt(batch[k] % np.array(qs, dtype=object)[:, None], qs) for k in range(3)])
            truth = vector_round(X, Q, t)
            assert true_round(int(X[1, 0]), Q, t)[0] == int(truth[1, 0])
            assert np.array_equal(m_want[~band], truth[~band])
            assert all(int(a) in (int(b), (int(b) - 1) % t) for a, b in zip(m_want[band], truth[band]))
            for offset in (0, 1):
                dx = object_words(g, batch, bits, offset)
                msg = filled(bits, 3 * n + 16, offset, GUARD)
                worst = filled(bits, 3 + 16, 0, GUARD)
                with g.launch_log() as log:
                    plan.decode(dx, msg[:-16], worst[:-16], 3)
                torch.cuda.synchronize()
                assert log.kernels == ["bfv_decode"]
                got = host(g, msg[:3 * n], (3, n))
                assert np.array_equal(got, m_want), (t, name, offset)
                assert np.array_equal(got[~band], truth[~band])
                assert np.array_equal(host(g, worst[:3], (3,)), noise_max(n_want)), (t, name, offset)
                assert (g.to_host(msg[3 * n:]) == GUARD).all() and (g.to_host(worst[3:]) == GUARD).all()
                assert np.array_equal(host(g, dx, batch.shape), batch)
                # without noise_max: the same messages, one launch, nothing else written
                msg2 = filled(bits, 3 * n + 16, offset, GUARD)
                with g.launch_log() as log:
                    plan.decode(dx, msg2[:-16], None, 3)
                torch.cuda.synchronize()
                assert log.kernels == ["bfv_decode"]
                assert torch.equal(msg2, msg)
                # the two-launch form: partial maxima and bfv_decode_merge, no memset -- noise_max starts as garbage
                msg3 = filled(bits, 3 * n + 16, offset, GUARD)
                worst3 = filled(bits, 3 + 16, 0, GUARD)
                pbytes = plan.decode_partials_bytes(3)
                assert pbytes == -(-3 * max(1, n // 256) * (bits // 8) // 256) * 256
                part = filled(bits, pbytes // (bits // 8) + 16, 0, GUARD)
                with g.launch_log() as log:
                    plan.decode(dx, msg3[:-16], worst3[:-16], 3, partials=part[:-16])
                torch.cuda.synchronize()
                assert log.kernels == ["bfv_decode", "bfv_decode_merge"]
                assert torch.equal(msg3, msg) and torch.equal(worst3, worst), (t, name, offset)
                assert (g.to_host(part[-16:]) == GUARD).all()
            if name == "leak" and big >= 64:  # the three maxima differ: none has leaked into another stack
                assert len({int(v) for v in noise_max(n_want)}) == 3


# ------------------------------------------------------------------------------------------------------ encrypt_public
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [5, 12])
def test_encrypt_public_every_word(g, bits, n_power):
    """pk (so also a) and the message of any words, small with the lift's edge values planted (INT32_MIN included), with
    and without a message, aligned and one word off alignment"""
    import torch
    L, K, alpha, count = 3, 2, 2, 3
    full = ring(g, bits, n_power, M=8, widths="wide")
    st = full.sub(list(range(L + K)))
    cases, plan = full.cases[:L], make_plan(g, st, L, alpha, n_power, bits)
    n, qs = 1 << n_power, st["moduli"][:L]
    rng = np.random.default_rng(n_power * bits)
    small = planted_errors(rng, (3, count, n))
    assert -(1 << 31) in small
    pk_w = any_words(g, rng, bits, 2 * L * n, qs)
    for with_message in (True, False):
        msg_w = any_words(g, rng, bits, count * L * n, qs) if with_message else None
        want = exact_encrypt_public(cases, from_words(pk_w, (2, L, n)), small,
                                    from_words(msg_w, (count, L, n)) if with_message else None)
        for offset in (0, 1):
            pk, d_small = device_words(g, pk_w, offset), small_device(small, offset)
            message = device_words(g, msg_w, offset) if with_message else None
            out = filled(bits, 2 * count * L * n + 16, offset, GUARD)
            with g.launch_log() as log:
                plan.encrypt_public(pk, d_small, message, out[:-16], count,
                                    scratch_of(plan.encrypt_public_scratch_bytes(count)))
            torch.cuda.synchronize()
            assert log.kernels[0] == "lift_small" and log.kernels[-1] == "encrypt_public_combine"
            assert log.kernels.count("lift_small") == 1 and log.kernels.count("encrypt_public_combine") == 1
            assert np.array_equal(host(g, out[:2 * count * L * n], want.shape), want), (with_message, offset)
            assert (g.to_host(out[2 * count * L * n:]) == GUARD).all()
            assert np.array_equal(g.to_host(pk), pk_w)
            assert np.array_equal(g.to_host(d_small, signed=True).reshape(small.shape), small)
    assert plan.encrypt_public_scratch_bytes(count) == -(-3 * count * L * n * (bits // 8) // 256) * 256


# ------------------------------------------------------------------------------------------------------------- decrypt
def decrypt_inputs(g, rng, bits, st_p, L, count, components, n):
    """ct and s of residues (both forms of decrypt are defined on them)"""
    qs = st_p["moduli"]
    dt = g.np_dtype(bits)
    ct = np.concatenate([rng.integers(0, qs[m], size=n, dtype=np.uint64).astype(dt)
                         for _ in range(components * count) for m in range(L)])
    s = np.concatenate([rng.integers(0, q, size=n, dtype=np.uint64).astype(dt) for q in qs])
    return ct, s


@pytest.mark.parametrize("bits", [64, 32])
def test_decrypt_is_phase_then_decode_and_replays_from_a_graph(g, bits):
    """word for word phase + decode for both input forms and both component counts; then decrypt captured once on one
    stream (the memset of noise_max is a node) and replayed with new data"""
    import torch
    n_power, L, count, t = 9, 3, 3, 65537
    n = 1 << n_power
    _, st_b, st_p, bfv = bfv_for(g, bits, n_power, L, t, None)
    ks = make_plan(g, st_p, L, 2, n_power, bits)
    rng = np.random.default_rng(bits)
    scratch = scratch_of(bfv.decrypt_scratch_bytes(count))
    assert bfv.decrypt_scratch_bytes(count) == -(-count * L * n * (bits // 8) // 256) * 256
    for components in (2, 3):
        for input_ntt in (True, False):
            ct_w, s_w = decrypt_inputs(g, rng, bits, st_p, L, count, components, n)
            ct, s = device_words(g, ct_w), device_words(g, s_w)
            ks_scratch = scratch_of(ks.phase_scratch_bytes(count, components, input_ntt))
            msg, worst = filled(bits, count * n, 0, GUARD), filled(bits, count, 0, GUARD)
            with g.launch_log() as log:
                bfv.decrypt(ct, ks, s, msg, worst, count, components, input_ntt, scratch,
                            None if input_ntt else ks_scratch)
            torch.cuda.synchronize()
            assert log.kernels.count("decrypt_phase") == 1 and log.kernels[-1] == "bfv_decode"
            ph = filled(bits, count * L * n)
            ks.phase(ct, s, ph, count, components, input_ntt, False, ks_scratch)
            msg2, worst2 = filled(bits, count * n, 0, 1), filled(bits, count, 0, 1)
            bfv.decode(ph, msg2, worst2, count)
            torch.cuda.synchronize()
            assert torch.equal(msg, msg2) and torch.equal(worst, worst2), (components, input_ntt)

    components, input_ntt = 3, False
    ct_w, s_w = decrypt_inputs(g, rng, bits, st_p, L, count, components, n)
    ct, s = device_words(g, ct_w), device_words(g, s_w)
    ks_scratch = scratch_of(ks.phase_scratch_bytes(count, components, input_ntt))
    msg, worst = filled(bits, count * n, 0, GUARD), filled(bits, count, 0, GUARD)

    def run(stream):
        bfv.decrypt(ct, ks, s, msg, worst, count, components, input_ntt, scratch, ks_scratch, stream=stream)
    st_ = torch.cuda.Stream()
    st_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st_):  # eager warm-up on the capture stream
        run(st_)
    st_.synchronize()
    allocs = g.alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st_):
        run(st_)
    for seed in (1, 2):
        nct, ns = decrypt_inputs(g, np.random.default_rng(seed), bits, st_p, L, count, components, n)
        ct.copy_(g.to_device(nct)), s.copy_(g.to_device(ns))
        msg.fill_(GUARD), worst.fill_(GUARD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        m_graph, w_graph = msg.clone(), worst.clone()
        msg.fill_(GUARD), worst.fill_(GUARD)
        run(None)
        torch.cuda.synchronize()
        assert torch.equal(m_graph, msg) and torch.equal(w_graph, worst), seed
    assert g.alloc_count() == allocs


# ----------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_arrives_before_a_launch(g):
    import torch
    bits, n_power, L, count, t = 64, 6, 3, 2, 65537
    n = 1 << n_power
    full, st_b, st_p, bfv = bfv_for(g, bits, n_power, L, t, None)
    ks = make_plan(g, st_p, L, 2, n_power, bits)
    rng = np.random.default_rng(1)
    ct_w, s_w = decrypt_inputs(g, rng, bits, st_p, L, count, 3, n)
    ct, s = device_words(g, ct_w), device_words(g, s_w)
    out = filled(bits, count * L * n)
    pbytes = ks.phase_scratch_bytes(count, 3, False)
    big = scratch_of(pbytes + 256)
    ps, words64 = big[:pbytes], big[:pbytes].view(torch.int64)
    small = small_device(planted_errors(rng, (3, count, n)))
    pk, msg_ntt = filled(bits, 2 * L * n), filled(bits, count * L * n)
    ct2 = filled(bits, 2 * count * L * n)
    ebytes = ks.encrypt_public_scratch_bytes(count)
    ebig = scratch_of(ebytes + 256)
    es = ebig[:ebytes]
    message, worst = filled(bits, count * n), filled(bits, count)
    dbytes = bfv.decrypt_scratch_bytes(count)
    dbig = scratch_of(dbytes + 256)
    ds = dbig[:dbytes]

    # zero counts launch nothing
    with g.launch_log() as log:
        ks.phase(ct, s, out, 0, 3, False, False, ps)
        ks.encrypt_public(pk, small, msg_ntt, ct2, 0, es)
        bfv.scale_message(message, out, 0, True)
        bfv.decode(out, message, worst, 0)
        bfv.decrypt(ct, ks, s, message, worst, 0, 3, False, ds, ps)
    assert log.kernels == []

    bare = g.KeySwitchPlan(st_p["moduli"][:L], st_p["moduli"][L:], 2, n_power, bits=bits)
    bare_bfv = g.BfvMultiplyPlan(st_b["moduli"][:L], st_b["moduli"][L:], t, n_power, bits=bits)
    # plans that do not match bfv: another q-modulus, another ring, another reduction polynomial, no transforms
    K_b = len(st_b["moduli"]) - L
    p_idx = list(range(L + K_b, L + K_b + 2))
    other = full.sub([0, 1, L + K_b + 2] + p_idx) if len(full.moduli) > L + K_b + 2 else None
    small_ring = ring(g, bits, n_power - 1, M=len(full.moduli))
    cyclic = ring(g, bits, n_power, M=len(full.moduli), poly=g.X_N_minus)
    mismatched = [make_plan(g, small_ring.sub(list(range(L)) + p_idx), L, 2, n_power - 1, bits),
                  make_plan(g, cyclic.sub(list(range(L)) + p_idx), L, 2, n_power, bits), bare]
    if other is not None:
        mismatched.append(make_plan(g, other, L, 2, n_power, bits))
    # t >= some q_i; t >= 2^(W-2) cannot be below a prime of W - 2 bits, so the same message covers it
    q0 = ring(g, bits, n_power, M=8).moduli[0]  # the ring bases() gives L = 1
    _, big_b, big_p, big_t = bfv_for(g, bits, n_power, 1, q0 + 2, None)
    assert big_b["moduli"][0] == q0 and q0 + 2 < 1 << (bits - 2)
    big_ks = make_plan(g, big_p, 1, 1, n_power, bits)

    ph, enc, sc, dec, dcr = ks.phase, ks.encrypt_public, bfv.scale_message, bfv.decode, bfv.decrypt
    refused = [lambda: ph(None, s, out, count, 3, False, False, ps),
               lambda: ph(ct, None, out, count, 3, False, False, ps),
               lambda: ph(ct, s, None, count, 3, False, False, ps),
               lambda: ph(ct, s, out, count, 3, False, False, None),                  # the scratch is needed
               lambda: ph(ct, s, out, count, 1, True, True),
               lambda: ph(ct, s, out, count, 4, True, True),
               lambda: ph(ct, s, out, -1, 3, True, True),
               lambda: ph(ct[1:], s, out, count, 3, True, True),                      # too short
               lambda: ph(ct, s, out[1:], count, 3, True, True),
               lambda: ph(ct, s[:L * n - 1], out, count, 3, True, True),
               lambda: ph(ct, s, ct[L * n:(count + 1) * L * n], count, 3, True, True),  # out inside ct, not ct itself
               lambda: ph(ct, s, ct, count, 3, False, False, ps),                     # out = ct in coefficient form
               lambda: ph(ct, out[:L * n], out, count, 3, True, True),                # s inside out
               lambda: ph(ct, s, out, count, 3, False, False, big[8:8 + pbytes]),     # not 256-byte aligned
               lambda: ph(ct, s, out, count, 3, False, False, ps[:-256]),             # too small
               lambda: ph(words64[:3 * count * L * n], s, out, count, 3, False, False, ps),  # the scratch over ct
               lambda: ph(ct, s, words64[:count * L * n], count, 3, False, False, ps),       # the scratch over out
               lambda: bare.phase(ct, s, out, count, 3, False, True, ps),             # no transforms
               lambda: bare.phase(ct, s, out, count, 3, True, False),
               lambda: enc(None, small, msg_ntt, ct2, count, es),
               lambda: enc(pk, None, msg_ntt, ct2, count, es),
               lambda: enc(pk, small, msg_ntt, None, count, es),
               lambda: enc(pk, small, msg_ntt, ct2, count, None),
               lambda: enc(pk, small, msg_ntt, ct2, -1, es),
               lambda: enc(pk[1:], small, msg_ntt, ct2, count, es),
               lambda: enc(pk, small[1:], msg_ntt, ct2, count, es),
               lambda: enc(pk, small, msg_ntt[1:], ct2, count, es),
               lambda: enc(pk, small, msg_ntt, ct2[1:], count, es),
               lambda: enc(pk, small.to(torch.int64), msg_ntt, ct2, count, es),
               lambda: enc(ct2[:2 * L * n], small, msg_ntt, ct2, count, es),          # pk inside out
               lambda: enc(pk, small, ct2[:count * L * n], ct2, count, es),           # the message inside out
               lambda: enc(pk, small, msg_ntt, ebig[:ebytes].view(torch.int64)[:2 * count * L * n], count, es),
               lambda: enc(pk, small, msg_ntt, ct2, count, ebig[8:8 + ebytes]),
               lambda: enc(pk, small, msg_ntt, ct2, count, es[:-256]),
               lambda: bare.encrypt_public(pk, small, msg_ntt, ct2, count, es),
               lambda: sc(None, out, count, True),
               lambda: sc(message, None, count, True),
               lambda: sc(message, out, -1, True),
               lambda: sc(message[1:], out, count, True),
               lambda: sc(message, out[1:], count, True),
               lambda: sc(out[:count * n], out, count, True),                         # the message inside out
               lambda: bare_bfv.scale_message(message, out, count, True),             # to_ntt without transforms
               lambda: dec(None, message, worst, count),
               lambda: dec(out, None, worst, count),
               lambda: dec(out, message, worst, -1),
               lambda: dec(out[1:], message, worst, count),
               lambda: dec(out, message[1:], worst, count),
               lambda: dec(out, message, worst[1:], count),
               lambda: dec(out, out[:count * n], worst, count),                       # x over message_out
               lambda: dec(out, message, out[:count], count),                         # x over noise_max
               lambda: dec(out, message, message[:count], count),                     # the outputs over each other
               lambda: dcr(None, ks, s, message, worst, count, 3, False, ds, ps),
               lambda: dcr(ct, ks, None, message, worst, count, 3, False, ds, ps),
               lambda: dcr(ct, ks, s, None, worst, count, 3, False, ds, ps),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, None, ps),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, ds, None),
               lambda: dcr(ct, ks, s, message, worst, -1, 3, False, ds, ps),
               lambda: dcr(ct, ks, s, message, worst, count, 5, False, ds, ps),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, dbig[8:8 + dbytes], ps),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, ds[:-256], ps),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, ds, big[8:8 + pbytes]),
               lambda: dcr(ct, ks, s, ct[:count * n], worst, count, 3, True, ds, None),     # message_out inside ct
               lambda: dcr(ct, ks, s, message, s[:count], count, 3, True, ds, None),         # noise_max inside s
               lambda: dcr(ct, ks, s, dbig[:dbytes].view(torch.int64)[:count * n], worst, count, 3, True, ds, None),
               lambda: dcr(ct, ks, s, message, worst, count, 3, False, ps[:dbytes], ps),   # the two scratches overlap
               lambda: dcr(ct, object(), s, message, worst, count, 3, False, ds, ps),
               lambda: bare_bfv.decrypt(ct, ks, s, message, worst, count, 3, False, ds, ps)]
    refused += [lambda p=p: dcr(ct, p, s, message, worst, count, 3, False, ds, ps) for p in mismatched]
    unusable = [lambda: big_t.scale_message(message, filled(bits, count * n), count, False),
                lambda: big_t.decode(filled(bits, count * n), message, worst, count),
                lambda: big_t.decrypt(ct[:2 * count * n], big_ks, s, message, worst, count, 2, True, ds, None)]
    refused += unusable
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises((ValueError, RuntimeError)):
                f()
        assert log.kernels == [], i
    for p in mismatched[1:]:  # the message of multiply_relinearize
        with pytest.raises(ValueError, match="The key-switching plan does not match!"):
            dcr(ct, p, s, message, worst, count, 3, False, ds, ps)
    for f in unusable:
        with pytest.raises(ValueError, match="Plaintext modulus not usable here!"):
            f()
    torch.cuda.synchronize()


def test_the_library_itself_refuses_with_the_documented_messages(g):
    """the C ABI called directly, past the Python wrapper's own checks: every message the headers document, the grid limit
    and the int limit of the transforms' batch included.  A refusal comes before any access, so the operands are
    addresses that are never read: 256-byte aligned, far apart, backed by nothing"""
    import ctypes
    bits, n_power, L, t = 64, 6, 3, 65537
    _, st_b, st_p, bfv = bfv_for(g, bits, n_power, L, t, None)
    ks = make_plan(g, st_p, L, 2, n_power, bits)
    bare = g.KeySwitchPlan(st_p["moduli"][:L], st_p["moduli"][L:], 2, n_power, bits=bits)
    bare_bfv = g.BfvMultiplyPlan(st_b["moduli"][:L], st_b["moduli"][L:], t, n_power, bits=bits)
    lib = g.load_library()
    P = ctypes.c_void_p
    A, B, C, D, E, F = (P(k << 44) for k in range(1, 7))
    NULL = P(None)
    phase, public = lib.gpuntt_keyswitch_plan_phase_u64, lib.gpuntt_keyswitch_plan_encrypt_public_u64
    scale, decode, decrypt = (lib.gpuntt_bfv_plan_scale_message_u64, lib.gpuntt_bfv_plan_decode_u64,
                              lib.gpuntt_bfv_plan_decrypt_u64)
    two = lib.gpuntt_bfv_plan_decode_two_launch_u64
    big = 1 << 27   # big * 64 lanes pass HIP's 2^32 - 1 work-items; 3 * big * L still fits an int
    huge = 1 << 30  # count * L passes an int
    cases = [
        (lambda: phase(ks._h, NULL, B, C, 2, 2, 1, 1, NULL, NULL), "null pointer argument"),
        (lambda: phase(ks._h, A, NULL, C, 2, 2, 1, 1, NULL, NULL), "null pointer argument"),
        (lambda: phase(ks._h, A, B, NULL, 2, 2, 1, 1, NULL, NULL), "null pointer argument"),
        (lambda: phase(ks._h, A, B, C, 2, 2, 0, 0, NULL, NULL), "null pointer argument"),       # the scratch is needed
        (lambda: phase(ks._h, A, B, C, 2, 1, 1, 1, NULL, NULL), "Invalid components!"),
        (lambda: phase(ks._h, A, B, C, 2, 4, 1, 1, NULL, NULL), "Invalid components!"),
        (lambda: phase(ks._h, A, B, C, -1, 2, 1, 1, NULL, NULL), "Invalid count!"),
        (lambda: phase(ks._h, A, B, C, huge, 2, 1, 1, NULL, NULL), "Invalid count!"),            # the int limit
        (lambda: phase(ks._h, A, B, C, big, 2, 1, 1, NULL, NULL), "Invalid count!"),             # the grid limit
        (lambda: phase(ks._h, A, B, C, 2, 2, 0, 0, P((4 << 44) + 8), NULL), "The scratch is not 256-byte aligned!"),
        (lambda: phase(ks._h, A, B, P((1 << 44) + 8), 2, 2, 1, 1, NULL, NULL), "out overlaps an operand!"),
        (lambda: phase(ks._h, A, B, A, 2, 2, 0, 0, D, NULL), "out overlaps an operand!"),        # out = ct, coefficients
        (lambda: phase(ks._h, A, B, C, 2, 2, 0, 0, C, NULL), "The scratch overlaps out!"),
        (lambda: phase(bare._h, A, B, C, 2, 2, 1, 0, NULL, NULL), None),                         # no transforms
        (lambda: public(ks._h, NULL, B, C, D, 2, E, NULL), "null pointer argument"),
        (lambda: public(ks._h, A, B, C, D, 2, NULL, NULL), "null pointer argument"),
        (lambda: public(ks._h, A, B, C, D, -1, E, NULL), "Invalid count!"),
        (lambda: public(ks._h, A, B, C, D, huge, E, NULL), "Invalid count!"),
        (lambda: public(ks._h, A, B, C, D, big, E, NULL), "Invalid count!"),
        (lambda: public(ks._h, A, B, C, D, 2, P((5 << 44) + 8), NULL), "The scratch is not 256-byte aligned!"),
        (lambda: public(ks._h, A, B, D, D, 2, E, NULL), "out or the scratch overlaps an operand!"),
        (lambda: public(ks._h, A, B, C, D, 2, D, NULL), "The scratch overlaps out!"),
        (lambda: scale(bfv._h, NULL, B, 2, 0, NULL), "null pointer argument"),
        (lambda: scale(bfv._h, A, NULL, 2, 0, NULL), "null pointer argument"),
        (lambda: scale(bfv._h, A, B, -1, 0, NULL), "Invalid count!"),
        (lambda: scale(bfv._h, A, B, huge, 0, NULL), "Invalid count!"),
        (lambda: scale(bfv._h, A, B, big, 0, NULL), "Invalid count!"),
        (lambda: scale(bfv._h, A, A, 2, 0, NULL), "scale_message input and output overlap!"),
        (lambda: scale(bare_bfv._h, A, B, 2, 1, NULL), "The plan was built without transform tables!"),
        (lambda: decode(bfv._h, NULL, B, C, 2, NULL), "null pointer argument"),
        (lambda: decode(bfv._h, A, NULL, C, 2, NULL), "null pointer argument"),
        (lambda: decode(bfv._h, A, B, C, -1, NULL), "Invalid stacks!"),
        (lambda: decode(bfv._h, A, B, C, big, NULL), "Invalid stacks!"),                         # the grid limit
        (lambda: decode(bfv._h, A, A, C, 2, NULL), "decode input and output overlap!"),
        (lambda: decode(bfv._h, A, B, A, 2, NULL), "decode input and output overlap!"),
        (lambda: decode(bfv._h, A, B, B, 2, NULL), "decode input and output overlap!"),
        (lambda: two(bfv._h, A, B, C, 2, A, NULL), "decode input and output overlap!"),            # the partials over x
        (lambda: two(bfv._h, A, B, C, 2, C, NULL), "decode input and output overlap!"),            # ... over noise_max
        (lambda: two(bfv._h, A, B, C, -1, D, NULL), "Invalid stacks!"),
        (lambda: decrypt(bfv._h, A, bare._h, B, C, D, 2, 2, 1, E, NULL, NULL), "The key-switching plan does not match!"),
        (lambda: decrypt(bfv._h, A, ks._h, B, C, D, 2, 2, 1, NULL, NULL, NULL), "null pointer argument"),
        (lambda: decrypt(bfv._h, A, ks._h, B, NULL, D, 2, 2, 1, E, NULL, NULL), "null pointer argument"),
        (lambda: decrypt(bfv._h, NULL, ks._h, B, C, D, 2, 2, 1, E, NULL, NULL), "null pointer argument"),
        (lambda: decrypt(bfv._h, A, ks._h, B, C, D, -1, 2, 1, E, NULL, NULL), "Invalid count!"),
        (lambda: decrypt(bfv._h, A, ks._h, B, C, D, 2, 5, 1, E, NULL, NULL), "Invalid components!"),
        (lambda: decrypt(bfv._h, A, ks._h, B, C, D, 2, 2, 1, P((5 << 44) + 8), NULL, NULL),
         "The scratch is not 256-byte aligned!"),
        (lambda: decrypt(bfv._h, A, ks._h, B, A, D, 2, 2, 1, E, NULL, NULL), "out or the scratch overlaps an operand!"),
        (lambda: decrypt(bfv._h, A, ks._h, B, C, D, 2, 2, 0, E, NULL, NULL), "null pointer argument")]  # the phase's
    for i, (f, message) in enumerate(cases):
        with g.launch_log() as log:
            rc = f()
        assert rc != 0 and log.kernels == [], i
        got = lib.gpuntt_last_error().decode()
        assert message is None or got == message, (i, got, message)


# ------------------------------------------------------------------------------------------------- the loop closes
def sparse_product(m1, idx, val, t):
    """m1 * m2 mod (t, X^N + 1) for m2 = sum_k val[k] X^idx[k], in int64 (8 terms below t^2 each)"""
    n = len(m1)
    out = np.zeros(n, dtype=np.int64)
    for k, c in zip(idx, val):
        shifted = np.concatenate([-m1[n - k:], m1[:n - k]]) if k else m1.copy()
        out += int(c) * shifted
    return out % t


@pytest.mark.parametrize("bits", [64, 32])
def test_the_loop_closes_on_device_made_material(g, bits):
    """n_power 12, K = 2, alpha = 2; u64: L = 3, t = 65537; u32: L = 1, t = 2.  Everything made on the device: a ternary secret (sample_small,
    lift_small), a public key (encrypt_symmetric of zero with a uniform `a`), a relinearization key (s^2 by operator_gpu,
    generate_keys with cbd21 errors), uniform messages; scale_message -> encrypt_public (u ternary, e0 / e1 cbd21) ->
    decrypt returns the messages exactly; multiply_relinearize -> decrypt returns m1 m2 mod (t, X^N + 1) exactly.

    The parameters, and why.  decode reports the noise as a W-bit word n ~ 2^W v, so a budget above
    W - 1 - bit_length(3 L) bits reads as that cap: with the 60-bit primes of the other u64 tests the fresh v ~ 2^-140
    and the v after one multiplication ~ 2^-100 are both zero at that resolution and `after < fresh` would compare
    rounding slack.  u64: primes of 30, 29 and 28 bits (Q ~ 2^87); |E| ~ 2^10 in practice (2^17 at worst), so the fresh
    2^64 v ~ 2^(64 + 16 + 10 - 87) = 2^3 is just resolved and one multiplication (a factor t 2^10 or so) leaves ~ 33 bits.
    u32: a 32-bit word resolves at most 27 bits of budget and one multiplication at t = 65537 consumes about as many, so
    the u32 case takes the smallest t and one 30-bit prime (L = 1, the first L of the u32 BFV tests): fresh
    v ~ 2 * 2^10 / 2^30 = 2^-19 (budget ~ 17 bits), after one multiplication ~ 2^-8 (budget ~ 6 bits).

    The fresh bound, from the sampled magnitudes.  The phase is x = floor((Q m + h) / t) + E with
    E = e_pk u + e0 + e1 s (negacyclic), so |E| <= |e_pk|_inf |u|_1 + |e0|_inf + |e1|_inf |s|_1 =: B, and
    t x / Q = m + ((h - r) + t E) / Q with |h - r| <= t / 2: |v| <= t (B + 1/2) / Q.  decode's word obeys
    |n| <= 2^W |v| + 3 L, so noise_max <= 2^W t (B + 1/2) / Q + 3 L, which is asserted; the budget follows from it."""
    import torch
    n_power, K, alpha, count = 12, 2, 2, 2
    L, t = {64: (3, 65537), 32: (1, 2)}[bits]
    n = 1 << n_power
    full, st_b, st_p, bfv = bfv_for(g, bits, n_power, L, t, NARROW)
    ks = make_plan(g, st_p, L, alpha, n_power, bits)
    M, D = L + K, ks.digits
    qs, fullp = st_p["moduli"][:L], st_p["moduli"]
    Q = math.prod(qs)
    mods = [g.Modulus(q, bits=bits) for q in fullp]

    # the secret, s^2, the relinearization key, the public key
    s_small = filled(32, n)
    g.sample_small(s_small, 1, n_power, g.TERNARY, 101, 0)
    s_ntt = filled(bits, M * n)
    ks.lift_small(s_small, s_ntt, 1, True, True)
    s_sq = filled(bits, M * n)
    for m in range(M):
        s_sq[m * n:(m + 1) * n] = g.operator_gpu(2, s_ntt[m * n:(m + 1) * n], s_ntt[m * n:(m + 1) * n], mods[m])
    key = filled(bits, D * 2 * M * n)
    g.sample_uniform(key[M * n:], fullp, n_power, D, 102, 0, stack_stride_words=2 * M * n)
    key_err = filled(32, D * n)
    g.sample_small(key_err, D, n_power, g.CBD21, 103, 0)
    ks.generate_keys(s_ntt, s_sq, key_err, [key], scratch_of(ks.keygen_scratch_bytes(1)))
    pk = filled(bits, 2 * L * n)
    g.sample_uniform(pk[L * n:], qs, n_power, 1, 104, 0)
    e_pk = filled(32, n)
    g.sample_small(e_pk, 1, n_power, g.CBD21, 105, 0)
    ks.encrypt_symmetric(s_ntt, e_pk, None, pk, 1, scratch_of(ks.encrypt_scratch_bytes(1)))

    # the messages: m1 uniform modulo t on the device, m2 sparse
    msgs = filled(bits, count * n, 0, 0)
    g.sample_uniform(msgs[:n], [t], n_power, 1, 106, 0)
    rng = np.random.default_rng(bits)
    idx, val = rng.choice(n, size=8, replace=False), rng.integers(1, t, size=8)
    m2 = np.zeros(n, dtype=np.int64)
    m2[idx] = val
    msgs[n:] = g.to_device(m2.astype(g.np_dtype(bits)))
    scaled = filled(bits, count * L * n)
    bfv.scale_message(msgs, scaled, count, True)
    small = filled(32, 3 * count * n)
    g.sample_small(small[:count * n], count, n_power, g.TERNARY, 107, 0)
    g.sample_small(small[count * n:], 2 * count, n_power, g.CBD21, 108, 0)
    ct = filled(bits, 2 * count * L * n)
    ks.encrypt_public(pk, small, scaled, ct, count, scratch_of(ks.encrypt_public_scratch_bytes(count)))

    # fresh: decrypt returns the messages
    out_m, out_n = filled(bits, count * n), filled(bits, count)
    d_scratch = scratch_of(bfv.decrypt_scratch_bytes(count))
    bfv.decrypt(ct, ks, s_ntt, out_m, out_n, count, 2, True, d_scratch, None)
    torch.cuda.synchronize()
    assert torch.equal(out_m, msgs)
    fresh_noise = [int(v) for v in g.to_host(out_n)]
    budget_fresh = min(g.noise_budget_bits(v, L, bits) for v in fresh_noise)

    sm = g.to_host(small, signed=True).astype(np.int64).reshape(3, count, n)
    s_h, epk_h = g.to_host(s_small, signed=True).astype(np.int64), g.to_host(e_pk, signed=True).astype(np.int64)
    assert set(np.unique(s_h)) <= {-1, 0, 1} and np.abs(sm[1:]).max() <= 21 and np.abs(epk_h).max() <= 21
    bounds = []
    for r in range(count):
        B = int(np.abs(epk_h).max()) * int(np.abs(sm[0, r]).sum()) + int(np.abs(sm[1, r]).max()) + \
            int(np.abs(sm[2, r]).max()) * int(np.abs(s_h).sum())
        bounds.append(((1 << bits) * t * (2 * B + 1)) // (2 * Q) + 1 + 3 * L)

    # ct x ct, relinearized, decrypted
    x, y = filled(bits, 2 * L * n), filled(bits, 2 * L * n)
    v = ct.view(2, count, L * n)
    x.view(2, L * n).copy_(v[:, 0]), y.view(2, L * n).copy_(v[:, 1])
    prod = filled(bits, 2 * L * n)
    bfv.multiply_relinearize(x, y, ks, key, prod, 1, True, True, bfv_scratch(bfv, 1), scratch_of(ks.scratch_bytes(1, 2)))
    p_m, p_n = filled(bits, n), filled(bits, 1)
    bfv.decrypt(prod, ks, s_ntt, p_m, p_n, 1, 2, True, d_scratch, None)
    torch.cuda.synchronize()
    after_noise = int(g.to_host(p_n)[0])
    budget_after = g.noise_budget_bits(after_noise, L, bits)
    m1 = g.to_host(msgs[:n]).astype(np.int64)
    assert m1.max() < t
    want = sparse_product(m1, idx, val, t)
    text = "budget fresh %d bits (noise words %s, bounds %s), after one multiplication %d bits (noise word %d)" % (
        budget_fresh, fresh_noise, bounds, budget_after, after_noise)
    print(text)
    assert all(v <= b for v, b in zip(fresh_noise, bounds)), text
    assert np.array_equal(g.to_host(p_m).astype(np.int64), want), text
    assert 0 < budget_after < budget_fresh, text


def test_cpp_caller_of_the_public_headers(g):
    """tests/cpp/example_bfv_roundtrip.cpp, compiled here against include/ and libgpuntt.so: sampling, keys, scale_message,
    encrypt_public, multiply_relinearize and decrypt through the C++ interface, all on the device; it prints both noise
    budgets and its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_bfv_roundtrip")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_bfv_roundtrip.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
