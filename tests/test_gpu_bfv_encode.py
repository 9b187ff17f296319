"""BFV batching on the GPU (include/gpuntt/rns/bfv_encode.cuh; KeySwitchPlan.lift_centred / multiply_plain,
include/gpuntt/rns/key_switch.cuh, "Plaintext operands"): every output word against tests/encode_exact.py, the launch
sequence, round trips at rings 2^13 to 2^16, a hipGraph replay, every refusal before a launch -- and THE MEANING of the
evaluator calls on slots, on device-made material: a ct x ct product is the slot-wise product, GaloisElementForRotation(s)
rotates both rows left by s, conjugation swaps them, and linear_transform_bsgs computes a banded matrix-vector product."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from bfv_utils import bfv_scratch
from bfv_utils import make_plan as make_bfv_plan
from encode_exact import (exact_decode, exact_encode, exact_lift_centred, exact_multiply_plain, plain_factors,
                          rotate_rows, swap_rows)
from encode_utils import Encoder, plain_for_ring, widest_plain
from hoisted_utils import any_words, device_words, filled, make_plan, ring
from innerprod_utils import from_words
from relin3_utils import bases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
NARROW = (30, 29, 28, 27)  # the prime widths of the meaning test, for both word widths: the same Q
T = 65537


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    return pkg


def scratch_of(nbytes):
    import torch
    return torch.zeros(max(256, nbytes), dtype=torch.uint8, device="cuda:0")


def host(g, t, shape):
    return from_words(g.to_host(t), shape)


def object_words(g, x, bits, offset=0):
    """an object array of words -> a device tensor"""
    return device_words(g, np.ascontiguousarray(x.astype(np.uint64).astype(g.np_dtype(bits)).reshape(-1)), offset)


def plain_moduli(bits, n_power):
    """65537 and the widest NTT prime of the word, each with its roots for this ring"""
    return [plain_factors(T, n_power), widest_plain(bits, n_power)]


# ---------------------------------------------------------------------------------------------------- encode and decode
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
def test_encode_and_decode_every_word(g, bits, n_power):
    """count 3 (one lane, one workgroup, several workgroups); values of any words with the edges of t planted; the
    operands aligned and one word off alignment; guard words after every output, the inputs untouched; exactly one
    bfv_slot_permute before the inverse plan's kernels (encode) and after the forward plan's (decode)"""
    import torch
    n, count = 1 << n_power, 3
    for factors in plain_moduli(bits, n_power):
        enc = Encoder(g, bits, n_power, factors)
        t = enc.t
        rng = np.random.default_rng(bits + n_power + t % 1000)
        # what the two transforms launch on their own
        probe = filled(bits, count * n, 0, 0)
        launches = {}
        for name, table, kind, ninv in (("fwd", enc.case.fwd_dev, g.FORWARD, None),
                                        ("inv", enc.case.inv_dev, g.INVERSE, enc.case.prm.n_inv)):
            plan = g.NTTPlan(table, enc.case.prm.modulus, n_power, g.X_N_plus, kind, ninv)
            with g.launch_log() as log:
                plan.execute(probe, probe, count)
            launches[name] = log.kernels
        torch.cuda.synchronize()
        assert launches["fwd"] and launches["inv"]

        values_w = any_words(g, rng, bits, count * n, [t, t + 1, (t + 1) >> 1])
        plain_want = exact_encode(enc.case, from_words(values_w, (count, n)))
        plain_w = rng.integers(0, t, size=count * n, dtype=np.uint64).astype(g.np_dtype(bits))
        values_want = exact_decode(enc.case, from_words(plain_w, (count, n)))
        assert enc.plan.scratch_bytes(count) == -(-count * n * (bits // 8) // 256) * 256
        for offset in (0, 1):
            values = device_words(g, values_w, offset)
            plain = filled(bits, count * n + 16, offset, GUARD)
            with g.launch_log() as log:
                enc.plan.encode(values, plain[:-16], count)
            torch.cuda.synchronize()
            assert log.kernels == ["bfv_slot_permute"] + launches["inv"], (log.kernels, launches["inv"])
            assert np.array_equal(host(g, plain[:count * n], (count, n)), plain_want), (t, offset)
            assert (g.to_host(plain[count * n:]) == GUARD).all() and np.array_equal(g.to_host(values), values_w)

            coeffs = device_words(g, plain_w, offset)
            slots = filled(bits, count * n + 16, offset, GUARD)
            scratch = scratch_of(enc.plan.scratch_bytes(count) + 256)
            scratch.fill_(0x5A)
            with g.launch_log() as log:
                enc.plan.decode(coeffs, slots[:-16], count, scratch[:enc.plan.scratch_bytes(count)])
            torch.cuda.synchronize()
            assert log.kernels == launches["fwd"] + ["bfv_slot_permute"], (log.kernels, launches["fwd"])
            assert np.array_equal(host(g, slots[:count * n], (count, n)), values_want), (t, offset)
            assert (g.to_host(slots[count * n:]) == GUARD).all() and np.array_equal(g.to_host(coeffs), plain_w)
            assert (scratch[enc.plan.scratch_bytes(count):] == 0x5A).all()
        # a caller-owned workspace: the plan allocates nothing
        ws = scratch_of(g.BfvBatchEncoder.workspace_bytes(n_power, bits))
        mine = Encoder(g, bits, n_power, factors, workspace=ws)
        assert not mine.plan.owns_workspace and enc.plan.owns_workspace
        plain = filled(bits, count * n)
        mine.plan.encode(device_words(g, values_w), plain, count)
        torch.cuda.synchronize()
        assert np.array_equal(host(g, plain, (count, n)), plain_want)


@pytest.mark.parametrize("bits,n_power", [(64, 13), (32, 14), (64, 15), (32, 15), (64, 16), (32, 16)])
def test_round_trip_at_larger_rings(g, bits, n_power):
    """decode(encode(v)) = v mod t, count 2; at 2^16 t = 1 mod 2^17 comes from find_ntt_factors"""
    import torch
    n, count = 1 << n_power, 2
    factors = plain_for_ring(n_power)
    t = factors[0]
    assert (t - 1) % (2 * n) == 0
    enc = Encoder(g, bits, n_power, factors)
    rng = np.random.default_rng(n_power)
    values_w = any_words(g, rng, bits, count * n, [t])
    values, plain, back = device_words(g, values_w), filled(bits, count * n), filled(bits, count * n)
    enc.plan.encode(values, plain, count)
    enc.plan.decode(plain, back, count, scratch_of(enc.plan.scratch_bytes(count)))
    torch.cuda.synchronize()
    assert np.array_equal(g.to_host(back), values_w % np.array(t, dtype=values_w.dtype))
    assert int(g.to_host(plain).max()) < t


# ------------------------------------------------------------------------------------------------------- lift_centred
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
def test_lift_centred_every_word(g, bits, n_power):
    """both bases, both forms, aligned and one word off; t = 65537 and the widest prime of the word, which exceeds some
    limbs' moduli; the words any value with (t + 1) >> 1 - 1, (t + 1) >> 1, t - 1 and t planted; one lift_centred, then
    exactly what lift_small's transform launches"""
    import torch
    L, K, alpha, polys = 3, 2, 2, 3
    full = ring(g, bits, n_power, M=8, widths="wide")
    st = full.sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    n, M = 1 << n_power, L + K
    for t in (T, widest_plain(bits, n_power)[0], 2):
        rng = np.random.default_rng(bits + n_power + t % 1000)
        up = (t + 1) >> 1
        words_w = any_words(g, rng, bits, polys * n, [up, up + 1, t, t + 1, t + up])
        if n_power >= 5:
            assert {up - 1, up, t - 1, t} <= {int(v) for v in words_w}
        if t > T:
            assert any(t > q for q in st["moduli"])
        for full_base in (True, False):
            B = M if full_base else L
            cases = full.cases[:B]
            for to_ntt in (False, True):
                want = exact_lift_centred(cases, t, from_words(words_w, (polys, n)), to_ntt)
                small = filled(32, polys * n, 0, 0)
                with g.launch_log() as log:
                    plan.lift_small(small, filled(bits, polys * B * n), polys, full_base, to_ntt)
                tail = log.kernels[1:]
                for offset in (0, 1):
                    words = device_words(g, words_w, offset)
                    out = filled(bits, polys * B * n + 16, offset, GUARD)
                    with g.launch_log() as log:
                        plan.lift_centred(words, t, out[:-16], polys, full_base, to_ntt)
                    torch.cuda.synchronize()
                    assert log.kernels == ["lift_centred"] + tail and (len(tail) == 0) == (not to_ntt), log.kernels
                    key = (t, full_base, to_ntt, offset)
                    assert np.array_equal(host(g, out[:polys * B * n], want.shape), want), key
                    assert (g.to_host(out[polys * B * n:]) == GUARD).all(), key
                    assert np.array_equal(g.to_host(words), words_w), key


# ----------------------------------------------------------------------------------------------------- multiply_plain
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n_power", [1, 5, 12])
def test_multiply_plain_every_word(g, bits, n_power):
    """any words in both operands, a shared plaintext and one per ciphertext, aligned and one word off, and out = ct;
    one launch"""
    import torch
    L, K, alpha, count = 3, 2, 2, 3
    full = ring(g, bits, n_power, M=8, widths="wide")
    st = full.sub(list(range(L + K)))
    plan = make_plan(g, st, L, alpha, n_power, bits)
    n, qs = 1 << n_power, st["moduli"][:L]
    rng = np.random.default_rng(3 * bits + n_power)
    ct_w = any_words(g, rng, bits, 2 * count * L * n, qs)
    ct_h = from_words(ct_w, (2, count, L, n))
    for pc in (1, count):
        pt_w = any_words(g, rng, bits, pc * L * n, qs)
        want = exact_multiply_plain(qs, ct_h, from_words(pt_w, (pc, L, n)))
        for offset in (0, 1):
            ct, pt = device_words(g, ct_w, offset), device_words(g, pt_w, offset)
            out = filled(bits, 2 * count * L * n + 16, offset, GUARD)
            with g.launch_log() as log:
                plan.multiply_plain(ct, pt, out[:-16], count, pc)
            torch.cuda.synchronize()
            assert log.kernels == ["multiply_plain"]
            assert np.array_equal(host(g, out[:2 * count * L * n], want.shape), want), (pc, offset)
            assert (g.to_host(out[2 * count * L * n:]) == GUARD).all()
            assert np.array_equal(g.to_host(ct), ct_w) and np.array_equal(g.to_host(pt), pt_w)
            with g.launch_log() as log:
                plan.multiply_plain(ct, pt, ct, count, pc)  # in place
            torch.cuda.synchronize()
            assert log.kernels == ["multiply_plain"]
            assert np.array_equal(host(g, ct, want.shape), want) and np.array_equal(g.to_host(pt), pt_w), (pc, offset)
    # a plan without transforms multiplies as well
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], alpha, n_power, bits=bits)
    out = filled(bits, 2 * count * L * n)
    bare.multiply_plain(device_words(g, ct_w), device_words(g, pt_w), out, count, count)
    torch.cuda.synchronize()
    assert np.array_equal(host(g, out, want.shape), want)


# -------------------------------------------------------------------------------------------------- graph and refusals
@pytest.mark.parametrize("bits", [64, 32])
def test_encode_and_decode_replay_from_a_graph(g, bits):
    """both calls captured once on one stream and replayed with new data; nothing is allocated"""
    import torch
    n_power, count = 9, 3
    n = 1 << n_power
    enc = Encoder(g, bits, n_power, plain_factors(T, n_power))
    rng = np.random.default_rng(bits)
    values = device_words(g, any_words(g, rng, bits, count * n, [T]))
    plain, back = filled(bits, count * n, 0, GUARD), filled(bits, count * n, 0, GUARD)
    scratch = scratch_of(enc.plan.scratch_bytes(count))

    def run(stream):
        enc.plan.encode(values, plain, count, stream=stream)
        enc.plan.decode(plain, back, count, scratch, stream=stream)
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
        new = any_words(g, np.random.default_rng(seed), bits, count * n, [T])
        values.copy_(g.to_device(new))
        plain.fill_(GUARD), back.fill_(GUARD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        p_graph, b_graph = plain.clone(), back.clone()
        assert np.array_equal(host(g, p_graph, (count, n)), exact_encode(enc.case, from_words(new, (count, n)))), seed
        assert np.array_equal(g.to_host(b_graph), new % np.array(T, dtype=new.dtype)), seed
        plain.fill_(GUARD), back.fill_(GUARD)
        run(None)
        torch.cuda.synchronize()
        assert torch.equal(p_graph, plain) and torch.equal(b_graph, back), seed
    assert g.alloc_count() == allocs


def test_every_refusal_arrives_before_a_launch(g):
    import torch
    bits, n_power, L, count = 64, 6, 3, 2
    n = 1 << n_power
    enc = Encoder(g, bits, n_power, plain_factors(T, n_power))
    full = ring(g, bits, n_power, M=8)
    st = full.sub(list(range(L + 2)))
    ks = make_plan(g, st, L, 2, n_power, bits)
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], 2, n_power, bits=bits)
    M = L + 2
    values, plain = filled(bits, count * n), filled(bits, count * n, 0, 0)
    sbytes = enc.plan.scratch_bytes(count)
    big = scratch_of(sbytes + 256)
    scr, words64 = big[:sbytes], big[:sbytes].view(torch.int64)
    out_full, ct = filled(bits, count * M * n), filled(bits, 2 * count * L * n)
    pt, ct2 = filled(bits, count * L * n), filled(bits, 2 * count * L * n)

    with g.launch_log() as log:  # zero counts launch nothing
        enc.plan.encode(values, plain, 0)
        enc.plan.decode(plain, values, 0, scr)
        ks.lift_centred(values, T, out_full, 0, True, True)
        ks.multiply_plain(ct, pt, ct2, 0, 1)
    assert log.kernels == []

    e, d, lc, mp = enc.plan.encode, enc.plan.decode, ks.lift_centred, ks.multiply_plain
    refused = [lambda: e(None, plain, count),
               lambda: e(values, None, count),
               lambda: e(values, plain, -1),
               lambda: e(values[1:], plain, count),                      # too short
               lambda: e(values, plain[1:], count),
               lambda: e(values, values, count),                         # in place
               lambda: e(plain[:n], plain[n - 1:], 1),                   # one shared word
               lambda: e(values.to(torch.int32), plain, count),
               lambda: d(None, values, count, scr),
               lambda: d(plain, None, count, scr),
               lambda: d(plain, values, count, None),
               lambda: d(plain, values, -1, scr),
               lambda: d(plain[1:], values, count, scr),
               lambda: d(plain, values[1:], count, scr),
               lambda: d(plain, plain, count, scr),
               lambda: d(plain, values, count, big[8:8 + sbytes]),       # not 256-byte aligned
               lambda: d(plain, values, count, scr[:-256]),              # too small
               lambda: d(words64[:count * n], values, count, scr),       # the scratch over plain
               lambda: d(plain, words64[:count * n], count, scr),        # the scratch over values
               lambda: lc(None, T, out_full, count, True, True),
               lambda: lc(values, T, None, count, True, True),
               lambda: lc(values, T, out_full, -1, True, True),
               lambda: lc(values, 0, out_full, count, True, True),
               lambda: lc(values, 1, out_full, count, True, True),
               lambda: lc(values, 1 << 63, out_full, count, True, True),
               lambda: lc(values, (1 << 62) + 1, out_full, count, True, True),   # Modulus<T> refuses it
               lambda: lc(values[1:], T, out_full, count, True, True),
               lambda: lc(values, T, out_full[1:], count, True, True),
               lambda: lc(values, T, out_full[:count * L * n], count, True, True),  # the q-base size for the full base
               lambda: lc(out_full[:count * n], T, out_full, count, True, True),    # the words inside out
               lambda: bare.lift_centred(values, T, out_full, count, True, True),   # to_ntt without transforms
               lambda: mp(None, pt, ct2, count, 1),
               lambda: mp(ct, None, ct2, count, 1),
               lambda: mp(ct, pt, None, count, 1),
               lambda: mp(ct, pt, ct2, -1, 1),
               lambda: mp(ct, pt, ct2, count, 0),
               lambda: mp(ct, pt, ct2, count, 3),
               lambda: mp(ct[1:], pt, ct2, count, 1),
               lambda: mp(ct, pt[1:], ct2, count, count),
               lambda: mp(ct, pt, ct2[1:], count, 1),
               lambda: mp(ct, pt, ct[L * n:], 1, 1),                     # out inside ct, not ct itself
               lambda: mp(ct, ct2[:L * n], ct2, count, 1)]               # the plaintext inside out
    for i, f in enumerate(refused):
        with g.launch_log() as log:
            with pytest.raises((ValueError, RuntimeError)):
                f()
        assert log.kernels == [], i
    # the constructor's refusals
    c = enc.case
    with pytest.raises(ValueError, match="Plaintext modulus does not support batching!"):
        g.BfvBatchEncoder(g.Modulus(12289, bits=bits), 13, c.fwd_dev.repeat(128), c.inv_dev.repeat(128), 1)
    with pytest.raises(ValueError, match="Invalid modulus!"):
        g.BfvBatchEncoder(g.Modulus(T, 17, 5, bits), n_power, c.fwd_dev, c.inv_dev, c.prm.n_inv)
    for bad in (0, 29):
        with pytest.raises(ValueError, match="Invalid n_power range!"):
            g.BfvBatchEncoder(c.prm.modulus, bad, c.fwd_dev, c.inv_dev, c.prm.n_inv)
    for fwd, inv in ((None, c.inv_dev), (c.fwd_dev, None)):
        with pytest.raises(ValueError, match="null pointer argument"):
            g.BfvBatchEncoder(c.prm.modulus, n_power, fwd, inv, c.prm.n_inv)
    torch.cuda.synchronize()


def test_the_library_itself_refuses_with_the_documented_messages(g):
    """the C ABI called directly, past the Python wrapper's own checks.  A refusal comes before any access, so the
    operands are addresses that are never read: 256-byte aligned, far apart, backed by nothing"""
    import ctypes
    bits, n_power, L = 64, 6, 3
    n = 1 << n_power
    enc = Encoder(g, bits, n_power, plain_factors(T, n_power))
    st = ring(g, bits, n_power, M=8).sub(list(range(L + 2)))
    ks = make_plan(g, st, L, 2, n_power, bits)
    bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], 2, n_power, bits=bits)
    lib = g.load_library()
    P = ctypes.c_void_p
    A, B, C, D = (P(k << 44) for k in range(1, 5))
    NULL = P(None)
    U = ctypes.c_uint64
    encode, decode = lib.gpuntt_bfv_encoder_encode_u64, lib.gpuntt_bfv_encoder_decode_u64
    lift, mult = lib.gpuntt_keyswitch_plan_lift_centred_u64, lib.gpuntt_keyswitch_plan_multiply_plain_u64
    create = lib.gpuntt_bfv_encoder_create_u64
    h, c = ctypes.c_void_p(), enc.case
    fwd, inv = P(c.fwd_dev.data_ptr()), P(c.inv_dev.data_ptr())
    big = 1 << 27   # big * 64 lanes pass HIP's 2^32 - 1 work-items
    huge = 1 << 30  # polys * M passes an int
    cases = [
        (lambda: encode(enc.plan._h, NULL, B, 2, NULL), "null pointer argument"),
        (lambda: encode(enc.plan._h, A, NULL, 2, NULL), "null pointer argument"),
        (lambda: encode(enc.plan._h, A, B, -1, NULL), "Invalid count!"),
        (lambda: encode(enc.plan._h, A, A, 2, NULL), "encode input and output overlap!"),
        (lambda: encode(enc.plan._h, A, P((1 << 44) + 8 * n), 2, NULL), "encode input and output overlap!"),
        (lambda: encode(NULL, A, B, 2, NULL), "null pointer argument"),
        (lambda: decode(enc.plan._h, NULL, B, 2, C, NULL), "null pointer argument"),
        (lambda: decode(enc.plan._h, A, NULL, 2, C, NULL), "null pointer argument"),
        (lambda: decode(enc.plan._h, A, B, 2, NULL, NULL), "null pointer argument"),
        (lambda: decode(enc.plan._h, A, B, -1, C, NULL), "Invalid count!"),
        (lambda: decode(enc.plan._h, A, B, 2, P((3 << 44) + 8), NULL), "The scratch is not 256-byte aligned!"),
        (lambda: decode(enc.plan._h, A, A, 2, C, NULL), "decode input and output overlap!"),
        (lambda: decode(enc.plan._h, A, B, 2, A, NULL), "The scratch overlaps an operand!"),
        (lambda: decode(enc.plan._h, A, B, 2, B, NULL), "The scratch overlaps an operand!"),
        (lambda: lift(ks._h, NULL, U(T), B, 2, 1, 1, NULL), "null pointer argument"),
        (lambda: lift(ks._h, A, U(T), NULL, 2, 1, 1, NULL), "null pointer argument"),
        (lambda: lift(ks._h, A, U(T), B, -1, 1, 1, NULL), "Invalid polys!"),
        (lambda: lift(ks._h, A, U(T), B, huge, 1, 1, NULL), "Invalid polys!"),                   # the int limit
        (lambda: lift(ks._h, A, U(T), B, big, 1, 0, NULL), "Invalid count!"),                    # the grid limit
        (lambda: lift(ks._h, A, U(0), B, 2, 1, 1, NULL), "Invalid plaintext modulus!"),
        (lambda: lift(ks._h, A, U(1), B, 2, 1, 1, NULL), "Invalid plaintext modulus!"),
        (lambda: lift(ks._h, A, U(1 << 63), B, 2, 1, 1, NULL), "Invalid plaintext modulus!"),
        (lambda: lift(ks._h, A, U((1 << 62) + 1), B, 2, 1, 1, NULL), "Invalid plaintext modulus!"),
        (lambda: lift(ks._h, A, U(T), A, 2, 1, 1, NULL), "The lift's input and output overlap!"),
        (lambda: lift(bare._h, A, U(T), B, 2, 1, 1, NULL), None),                                # no transforms
        (lambda: mult(ks._h, NULL, B, C, 2, 1, NULL), "null pointer argument"),
        (lambda: mult(ks._h, A, NULL, C, 2, 1, NULL), "null pointer argument"),
        (lambda: mult(ks._h, A, B, NULL, 2, 1, NULL), "null pointer argument"),
        (lambda: mult(ks._h, A, B, C, -1, 1, NULL), "Invalid count!"),
        (lambda: mult(ks._h, A, B, C, big, 1, NULL), "Invalid count!"),                          # the grid limit
        (lambda: mult(ks._h, A, B, C, 2, 0, NULL), "Invalid plain_count!"),
        (lambda: mult(ks._h, A, B, C, 2, 3, NULL), "Invalid plain_count!"),
        (lambda: mult(ks._h, A, B, P((1 << 44) + 8), 2, 1, NULL), "out overlaps an operand!"),
        (lambda: mult(ks._h, A, B, B, 2, 1, NULL), "out overlaps an operand!"),
        (lambda: create(ctypes.byref(h), g.Modulus(12289, bits=bits).c(), 13, fwd, inv, U(1), 16, NULL, NULL),
         "Plaintext modulus does not support batching!"),
        (lambda: create(ctypes.byref(h), g.Modulus(T, 17, 5, bits).c(), n_power, fwd, inv, U(1), 16, NULL, NULL),
         "Invalid modulus!"),
        (lambda: create(ctypes.byref(h), c.prm.modulus.c(), 0, fwd, inv, U(1), 16, NULL, NULL), "Invalid n_power range!"),
        (lambda: create(ctypes.byref(h), c.prm.modulus.c(), 29, fwd, inv, U(1), 16, NULL, NULL), "Invalid n_power range!"),
        (lambda: create(ctypes.byref(h), c.prm.modulus.c(), n_power, NULL, inv, U(1), 16, NULL, NULL),
         "null pointer argument"),
        (lambda: create(ctypes.byref(h), c.prm.modulus.c(), n_power, fwd, NULL, U(1), 16, NULL, NULL),
         "null pointer argument")]
    for i, (f, message) in enumerate(cases):
        with g.launch_log() as log:
            rc = f()
        assert rc != 0 and log.kernels == [], i
        got = lib.gpuntt_last_error().decode()
        assert message is None or got == message, (i, got, message)
    out = ctypes.c_uint64()
    assert lib.gpuntt_bfv_encoder_scratch_bytes_u64(n_power, -1, ctypes.byref(out)) != 0
    assert lib.gpuntt_last_error().decode() == "Invalid count!"
    assert lib.gpuntt_bfv_encoder_workspace_bytes_u64(0, ctypes.byref(out)) != 0
    assert lib.gpuntt_last_error().decode() == "Invalid n_power range!"


# --------------------------------------------------------------------------------------------------------- the meaning
def narrow_plans(g, bits, n_power, L, t):
    """the ring's first L narrow primes, the smallest auxiliary base behind them and two special primes: the same moduli
    for both word widths"""
    _, st_b, st_p, _ = bases(g, bits, n_power, L, t, widths=NARROW)
    return st_b, st_p, make_bfv_plan(g, st_b, L, t, n_power, bits), make_plan(g, st_p, L, 2, n_power, bits)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_evaluator_calls_mean_what_they_say_on_slots(g, bits):
    """n_power 12, t = 65537, L = 3, K = 2, alpha = 2, the narrow primes, everything made on the device (a ternary secret,
    a public key, a relinearization key and ten Galois keys from s_from = GPU_Automorphism_NTT(s, k)).  With uniform slot
    vectors u, v, every comparison exact:
      1. encode -> scale_message -> encrypt_public -> decrypt -> decode returns u and v
      2. multiply_relinearize decodes to u (.) v mod t
      3. multiply_plain with lift_centred(encode(v)) decodes to u (.) v mod t
      4. rotate_hoisted by +1, -1, +7 and conjugation decodes to both rows rotated LEFT by the step, and to the rows swapped
      5. linear_transform_bsgs with n1 = n2 = 4 and sixteen diagonals d_j, each pre-rotated RIGHT by its giant step 4 g as
         the header's convention requires, decodes to out[r][c] = sum_j d_j[r][c] u[r][(c + j) mod N/2] mod t.
    Noise: |pt| <= 2^15 after the centred lift, N = 2^12, sixteen terms on a fresh noise below 2^17 stay below 2^50, far
    below Q / (2 t) ~ 2^70; no case is skipped or tolerated.  No noise budget is asserted here (test_gpu_decrypt.py's
    subject)."""
    import torch
    n_power, L, K, count = 12, 3, 2, 2
    n, half = 1 << n_power, 1 << (n_power - 1)
    st_b, st_p, bfv, ks = narrow_plans(g, bits, n_power, L, T)
    M, D = L + K, ks.digits
    qs, fullp = st_p["moduli"][:L], st_p["moduli"]
    assert [q.bit_length() for q in qs] == [30, 29, 28] and D == 2
    enc = Encoder(g, bits, n_power, plain_factors(T, n_power))
    mods = [g.Modulus(q, bits=bits) for q in fullp]
    rot = g.galois_element_for_rotation

    # the secret, the public key, the relinearization key
    s_small = filled(32, n)
    g.sample_small(s_small, 1, n_power, g.TERNARY, 201, 0)
    s_ntt = filled(bits, M * n)
    ks.lift_small(s_small, s_ntt, 1, True, True)
    s_sq = filled(bits, M * n)
    for m in range(M):
        s_sq[m * n:(m + 1) * n] = g.operator_gpu(2, s_ntt[m * n:(m + 1) * n], s_ntt[m * n:(m + 1) * n], mods[m])
    pk = filled(bits, 2 * L * n)
    g.sample_uniform(pk[L * n:], qs, n_power, 1, 204, 0)
    e_pk = filled(32, n)
    g.sample_small(e_pk, 1, n_power, g.CBD21, 205, 0)
    ks.encrypt_symmetric(s_ntt, e_pk, None, pk, 1, scratch_of(ks.encrypt_scratch_bytes(1)))

    # the keys: s^2, then sigma_k(s) for the rotations of case 4 and the steps of case 5, all in one generate_keys
    steps = [1, -1, 7, 2, 3, 4, 8, 12]
    elements = [rot(s, n_power) for s in steps] + [g.galois_element_for_conjugation(n_power)]
    s_from = filled(bits, (1 + len(elements)) * M * n)
    s_from[:M * n] = s_sq
    g.GPU_Automorphism_NTT(s_ntt, s_from[M * n:], elements, n_power, g.X_N_plus, M)
    keys = [filled(bits, D * 2 * M * n) for _ in range(1 + len(elements))]
    for i, key in enumerate(keys):
        g.sample_uniform(key[M * n:], fullp, n_power, D, 300 + i, 0, stack_stride_words=2 * M * n)
    key_err = filled(32, len(keys) * D * n)
    g.sample_small(key_err, len(keys) * D, n_power, g.CBD21, 203, 0)
    ks.generate_keys(s_ntt, s_from, key_err, keys, scratch_of(ks.keygen_scratch_bytes(len(keys))))
    relin = keys[0]
    key_of = dict(zip(steps + ["conj"], keys[1:]))
    elt_of = dict(zip(steps + ["conj"], elements))

    # 1. encode, encrypt, decrypt, decode
    rng = np.random.default_rng(bits)
    uv = rng.integers(0, T, size=(count, n), dtype=np.int64)
    u, v = uv[0].astype(object), uv[1].astype(object)
    values = g.to_device(uv.astype(g.np_dtype(bits)).reshape(-1))
    plain = filled(bits, count * n)
    enc.plan.encode(values, plain, count)
    scaled = filled(bits, count * L * n)
    bfv.scale_message(plain, scaled, count, True)
    small = filled(32, 3 * count * n)
    g.sample_small(small[:count * n], count, n_power, g.TERNARY, 207, 0)
    g.sample_small(small[count * n:], 2 * count, n_power, g.CBD21, 208, 0)
    ct = filled(bits, 2 * count * L * n)
    ks.encrypt_public(pk, small, scaled, ct, count, scratch_of(ks.encrypt_public_scratch_bytes(count)))
    d_scratch = scratch_of(bfv.decrypt_scratch_bytes(count))
    e_scratch = scratch_of(enc.plan.scratch_bytes(count))

    def slots_of(c, stacks=1):
        """decrypt `stacks` two-component ciphertexts in NTT form and decode them: [stacks][N] Python integers"""
        msg, out, worst = filled(bits, stacks * n), filled(bits, stacks * n), filled(bits, stacks)
        bfv.decrypt(c, ks, s_ntt, msg, worst, stacks, 2, True, d_scratch, None)
        enc.plan.decode(msg, out, stacks, e_scratch)
        torch.cuda.synchronize()
        return host(g, out, (stacks, n))

    got = slots_of(ct, count)
    assert np.array_equal(got[0], u) and np.array_equal(got[1], v)

    # 2. ct x ct is the slot-wise product
    x, y = filled(bits, 2 * L * n), filled(bits, 2 * L * n)
    view = ct.view(2, count, L * n)
    x.view(2, L * n).copy_(view[:, 0]), y.view(2, L * n).copy_(view[:, 1])
    prod = filled(bits, 2 * L * n)
    bfv.multiply_relinearize(x, y, ks, relin, prod, 1, True, True, bfv_scratch(bfv, 1), scratch_of(ks.scratch_bytes(1, 2)))
    assert np.array_equal(slots_of(prod)[0], (u * v) % T)

    # 3. ct x pt with the centred lift of encode(v)
    pt = filled(bits, L * n)
    ks.lift_centred(plain[n:], T, pt, 1, False, True)
    cp = filled(bits, 2 * L * n)
    ks.multiply_plain(x, pt, cp, 1, 1)
    assert np.array_equal(slots_of(cp)[0], (u * v) % T)

    # 4. rotations and conjugation of the ciphertext of u
    a = filled(bits, D * M * n)
    ks.decompose(x[L * n:], a, 1, True, scratch_of(ks.scratch_bytes(1, 1)))
    which = [1, -1, 7, "conj"]
    rotated = filled(bits, len(which) * 2 * L * n)
    ks.rotate_hoisted(a, x[:L * n], [key_of[w] for w in which], [elt_of[w] for w in which], rotated, 1, True,
                      scratch_of(ks.hoisted_scratch_bytes(1, len(which))))
    for i, w in enumerate(which):
        got = slots_of(rotated[i * 2 * L * n:(i + 1) * 2 * L * n])[0]
        want = swap_rows(u) if w == "conj" else rotate_rows(u, w)
        assert np.array_equal(got, want), w
    assert not np.array_equal(rotate_rows(u, 1), rotate_rows(u, -1))  # a wrong direction would show

    # 5. a banded matrix-vector product by baby steps and giant steps
    n1 = n2 = 4
    diag = rng.integers(0, T, size=(n1 * n2, n), dtype=np.int64).astype(object)
    pre = np.stack([rotate_rows(diag[j], -n1 * (j // n1)) for j in range(n1 * n2)])  # right by the giant step
    d_values = object_words(g, pre, bits)
    d_plain = filled(bits, n1 * n2 * n)
    enc.plan.encode(d_values, d_plain, n1 * n2)
    d_ntt = filled(bits, n1 * n2 * M * n)
    ks.lift_centred(d_plain, T, d_ntt, n1 * n2, True, True)
    weights = [[d_ntt[(gi * n1 + b) * M * n:(gi * n1 + b + 1) * M * n] for b in range(n1)] for gi in range(n2)]
    baby_keys = [None] + [key_of[b] for b in range(1, n1)]
    giant_keys = [None] + [key_of[n1 * gi] for gi in range(1, n2)]
    out = filled(bits, 2 * L * n)
    ks.linear_transform_bsgs(a, x[:L * n], x[L * n:], baby_keys, [rot(b, n_power) for b in range(n1)], giant_keys,
                             [rot(n1 * gi, n_power) for gi in range(n2)], weights, out, 1, True,
                             scratch_of(ks.bsgs_scratch_bytes(1, n1, n2)))
    want = np.zeros(n, dtype=object)
    for j in range(n1 * n2):
        want = (want + diag[j] * rotate_rows(u, j)) % T
    assert np.array_equal(slots_of(out)[0], want)
    assert half == n // 2 and math.prod(qs) // (2 * T) > 1 << 69


def test_cpp_caller_of_the_public_headers(g):
    """tests/cpp/example_bfv_slots.cpp, compiled here against include/ and libgpuntt.so: encode, encrypt, rotate and
    multiply, decrypt, decode through the C++ interface, all on the device; it prints its verdict"""
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "example_bfv_slots")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip",
                               os.path.join(ROOT, "tests", "cpp", "example_bfv_slots.cpp"),
                               "-O2", "-std=c++20", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                              timeout=300)
        r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "All Correct." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
