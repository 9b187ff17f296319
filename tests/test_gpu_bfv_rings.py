"""The BFV pipeline -- BfvMultiplyPlan (include/gpuntt/rns/bfv_multiply.cuh) with KeySwitchPlan's relinearize, key
material, phase and public-key encryption (include/gpuntt/rns/key_switch.cuh) and the samplers
(include/gpuntt/rns/sampling.cuh) -- on the MI355X at the ring sizes BFV runs at: N = 2^13 ... 2^16, u64 and u32.  What
tests/test_gpu_keyswitch_rings.py lists for the key-switching family above 2^12 is inherited here through the four other
NTTPlans a BfvMultiplyPlan builds over the base {q, b}, whose K_b grows with N by the size proof B >= 2 t N Q; on top
come the transform batches of this family (2 U count M forward, 3 count M inverse, 3 count L closing), bfv_decode's
reduction over up to 256 tiles, and scratch regions that alias by design and lie megabytes apart.

  1. the per-column kernels: every word against the library's host references where one exists, a fixed column sample
     (or everything, where that is cheap) against Python integers; 1 stack and count N = 2^17 columns; once per word size
     at 2^16 with every base pointer one word off 16-byte alignment.
  2. decode's noise maximum with the largest noise planted in a chosen tile, wave and lane of a chosen stack, in the
     one-launch form, the two-launch form and without noise_max; the most negative noise word and the band.
  3. multiply, multiply_relinearize, multiply_sum, multiply_relinearize_sum, relinearize, decrypt, generate_keys and
     encrypt_symmetric: every output word against the composition that defines each of them, counts 1 to 4, every form.
     At u64 2^16 the library's counter of four-polynomial-tile launches moves exactly for the eligible batches; at u64
     2^14 a plan pair built with batch_hint = 1 gives the words of the default pair.
  4. every entry point once per word size at 2^16 on the widest primes against exact Python integers: no GPU call and
     none of the library's arithmetic on the expected side.
  5. the closed loop on device-made material at 2^13 and 2^16, L = 3, t = 65537, with the noise of the result worked out
     in Python integers before the messages are compared.
  6. caller-owned workspaces and exact scratches between guard bytes, launch lists, one captured graph, all at 2^16.

Every comparison is equality of every output word unless stated; outputs are filled with -1 before each call and inputs
are compared with their copies afterwards.

Host-reference seconds of section 4, measured on the project's CPU machine at 2^16, count 1, on the primes of
hoisted_utils.WIDE_WIDTHS (62/61/60 bits at u64, 30/29/28 at u32), u64 / u32:
  multiply, NTT form in and out 6.0 / 3.2, coefficient form 4.3 / 2.9      multiply_relinearize 6.9 / 4.1
  multiply_sum, two terms 6.2 / 3.0                                          multiply_relinearize_sum 6.5 / 3.9
  relinearize, both forms 2.8 / 1.1        generate_keys, two keys 0.8 / 0.6      encrypt_symmetric 0.1 / 0.1
  encrypt_public 0.3 / 0.1                 phase, four calls 0.7 / 0.3           decrypt, two calls 0.5 / 0.3
Every case prints its own seconds."""
import itertools
import math
import time

import numpy as np
import pytest

from bfv_exact import exact_extend, exact_multiply, exact_scale_round
from bfv_rings_utils import (ALPHA, K_P, N_POWERS, Setup, decode_tiles, host, limbs, noisy_phase, object_words,
                             p4_groups, p4_multiply, p4_multiply_relinearize, p4_relinearize, plant, run_checked,
                             small_device, sparse_product, zeros_bytes)
from bfv_sum_exact import exact_multiply_relinearize_sum, exact_multiply_sum
from bfv_sum_utils import composition_bfv_sum, composition_multiply_sum, sum_scratch
from bfv_utils import bfv_scratch, composition_multiply, operands, reduced
from bfv_utils import make_plan as make_bfv_plan
from decrypt_exact import (combine_public, exact_decode, exact_encrypt_public, exact_phase, exact_scale_message,
                           noise_max, phase_words, true_round)
from decrypt_utils import usable
from hoisted_utils import any_words, canonical_key, device_words, filled, make_plan, tdtype
from innerprod_utils import from_words
from keygen_exact import combine_encrypt, combine_keys, exact_encrypt, exact_generate_keys, lift
from keygen_utils import planted_errors
from keyswitch_utils import centre, column_sample, columns_of, crt, guarded, guards_intact, unmodified
from relin3_exact import exact_bfv_multiply_relinearize, exact_mod_down_add, exact_relinearize
from relin3_utils import composition_bfv, composition_relinearize, relin3_operands
from relin_utils import relin_scratch
from sampling_exact import small_word, uniform_word

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 4)
FORMS = list(itertools.product((False, True), repeat=2))
PLAIN = 65537  # usable for scale_message / decode on every base of this file
SUM_PAIRS = [(0, 1), (0, 2)]  # two terms that share their x: U = 3 distinct operands

# (bits, n_power, prime set, L): every ring on the default and the widest primes (hoisted_utils.WIDE_WIDTHS), 45-bit
# primes at u64 2^16, L = 6 (three digits, ragged tail of the auxiliary conversion) once per word size
RING_CASES = [(bits, n_power, kind, 3) for bits in (64, 32) for n_power in N_POWERS for kind in ("default", "wide")]
RING_CASES += [(64, 16, "narrow", 3), (64, 16, "default", 6), (32, 16, "default", 6)]
rings = pytest.mark.parametrize("bits,n_power,kind,L", RING_CASES,
                                ids=["u%d-2^%d-%s-L%d" % c for c in RING_CASES])
SIZES = [(bits, n_power) for bits in (64, 32) for n_power in N_POWERS]
sizes = pytest.mark.parametrize("bits,n_power", SIZES, ids=["u%d-2^%d" % c for c in SIZES])


@pytest.fixture(scope="module")
def g(pkg):
    pkg.load_library()
    yield pkg
    pkg.set_test_hook("contig_p4", "1")


def big_count(n_power):
    return (1 << 17) >> n_power


def report_p4(s, deltas):
    if s.p4:
        print("contig_p4 launches per call at u64 2^16 (%s primes, L = %d): %s" % (s.kind, s.L, deltas))


# ----------------------------------------------------------------------------- 1. the per-column kernels at real sizes
@sizes
def test_extend_scale_round_and_mod_down_add_every_word_and_a_python_integer_column_sample(g, bits, n_power):
    """1 stack and count N = 2^17 columns; inputs of any words with 0, 2^W - 1, q - 1 and q planted"""
    import torch
    s = Setup(g, bits, n_power, "default")
    L, n, dt, t = s.L, s.n, g.np_dtype(bits), s.t
    qs, bs, ps, M = s.qs, s.qb[L:], s.qp[L:], s.M_b
    rng = np.random.default_rng(1000 * n_power + bits)
    for stacks in (1, big_count(n_power)):
        cols = column_sample(stacks * n, n_power + stacks)
        hx = any_words(g, rng, bits, stacks * L * n, qs)
        x, full = device_words(g, hx), filled(bits, stacks * M * n)
        with g.launch_log() as log:
            s.bfv.extend(x, full, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_extend"]
        got = g.to_host(full)
        want = g.bfv_reference_extend(qs, bs, hx, np.zeros(stacks * M * n, dtype=dt), n_power, stacks, bits)
        assert np.array_equal(got, want), ("extend", stacks)
        exact = exact_extend(qs, bs, columns_of(hx, 1, stacks, L, n, cols), bits)
        assert np.array_equal(columns_of(got, 1, stacks, M, n, cols), exact), ("extend columns", stacks)
        assert np.array_equal(g.to_host(x), hx), "in modified"

        hf = any_words(g, rng, bits, stacks * M * n, s.qb)
        f, out = device_words(g, hf), filled(bits, stacks * L * n)
        with g.launch_log() as log:
            s.bfv.scale_round(f, out, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_scale_round"]
        got = g.to_host(out)
        want = g.bfv_reference_scale_round(qs, bs, t, hf, np.zeros(stacks * L * n, dtype=dt), n_power, stacks, bits)
        assert np.array_equal(got, want), ("scale_round", stacks)
        exact = exact_scale_round(qs, bs, t, columns_of(hf, 1, stacks, M, n, cols), bits)
        assert np.array_equal(columns_of(got, 1, stacks, L, n, cols), exact), ("scale_round columns", stacks)
        assert np.array_equal(g.to_host(f), hf), "full modified"

        Mp = s.M_p
        hy, ha = any_words(g, rng, bits, stacks * Mp * n, s.qp), any_words(g, rng, bits, stacks * L * n, qs)
        y, addend, out = device_words(g, hy), device_words(g, ha), filled(bits, stacks * L * n)
        with g.launch_log() as log:
            s.ks.mod_down_add(y, addend, out, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["mod_down_add"]
        got = g.to_host(out)
        qv = np.array(qs, dtype=dt)[None, :, None]
        yres = np.ascontiguousarray((hy.reshape(stacks, Mp, n) % np.array(s.qp, dtype=dt)[None, :, None]).reshape(-1))
        down = g.keyswitch_reference_mod_down(qs, ps, yres, np.zeros(stacks * L * n, dtype=dt), n_power, stacks, bits)
        want = (down.reshape(stacks, L, n) + ha.reshape(stacks, L, n) % qv) % qv  # both below q < 2^(W-2): no wrap
        assert np.array_equal(got, want.reshape(-1)), ("mod_down_add", stacks)
        exact = exact_mod_down_add(qs, ps, columns_of(hy, 1, stacks, Mp, n, cols), columns_of(ha, 1, stacks, L, n, cols),
                                   bits)
        assert np.array_equal(columns_of(got, 1, stacks, L, n, cols), exact), ("mod_down_add columns", stacks)
        assert np.array_equal(g.to_host(y), hy) and np.array_equal(g.to_host(addend), ha), "an input was modified"


@sizes
def test_scale_message_decode_phase_and_lift_small_every_word_against_python_integers(g, bits, n_power):
    """the kernels that need no transform, on everything: scale_message and lift_small in coefficient form, decode of any
    words, phase in NTT form in and out with 2 and 3 components"""
    import torch
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, t, qs = s.L, s.n, s.t, s.qs
    assert usable(t, qs, bits)
    rng = np.random.default_rng(2000 * n_power + bits)
    for stacks in (1, big_count(n_power)):
        msg_w = any_words(g, rng, bits, stacks * n, [t, t + 1, 1])
        msg, out = device_words(g, msg_w), filled(bits, stacks * L * n)
        with g.launch_log() as log:
            s.bfv.scale_message(msg, out, stacks, False)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_scale_message"]
        want = exact_scale_message(qs, t, from_words(msg_w, (stacks, n)))
        assert np.array_equal(host(g, out, want.shape), want), ("scale_message", stacks)
        assert np.array_equal(g.to_host(msg), msg_w), "message modified"

        xw = any_words(g, rng, bits, stacks * L * n, qs)
        x, m_out, worst = device_words(g, xw), filled(bits, stacks * n), filled(bits, stacks)
        with g.launch_log() as log:
            s.bfv.decode(x, m_out, worst, stacks)
        torch.cuda.synchronize()
        assert log.kernels == ["bfv_decode"]
        m_want, n_want, _ = exact_decode(qs, t, from_words(xw, (stacks, L, n)), bits)
        assert np.array_equal(host(g, m_out, m_want.shape), m_want), ("decode", stacks)
        assert np.array_equal(host(g, worst, (stacks,)), noise_max(n_want)), ("noise_max", stacks)
        assert np.array_equal(g.to_host(x), xw), "x modified"

        small = planted_errors(rng, (stacks, n))
        d_small = small_device(small)
        for full_base in (False, True):
            mods = s.qp if full_base else qs
            out = filled(bits, stacks * len(mods) * n)
            with g.launch_log() as log:
                s.ks.lift_small(d_small, out, stacks, full_base, False)
            torch.cuda.synchronize()
            assert log.kernels == ["lift_small"]
            want = lift(mods, small)
            assert np.array_equal(host(g, out, want.shape), want), ("lift_small", stacks, full_base)
        assert np.array_equal(g.to_host(d_small, signed=True).reshape(small.shape), small)

        s_w = any_words(g, rng, bits, s.M_p * n, s.qp)
        sec = device_words(g, s_w)
        for components in (2, 3):
            ct_w = any_words(g, rng, bits, components * stacks * L * n, qs)
            ct, out = device_words(g, ct_w), filled(bits, stacks * L * n)
            with g.launch_log() as log:
                s.ks.phase(ct, sec, out, stacks, components, True, True)
            torch.cuda.synchronize()
            assert log.kernels == ["decrypt_phase"]
            want = phase_words(qs, from_words(ct_w, (components, stacks, L, n)), from_words(s_w, (s.M_p, n)))
            assert np.array_equal(host(g, out, want.shape), want), ("phase", stacks, components)
            assert np.array_equal(g.to_host(ct), ct_w) and np.array_equal(g.to_host(sec), s_w)


@sizes
def test_the_samplers_every_word_and_the_philox_model_on_a_column_sample(g, bits, n_power):
    """sample_uniform and sample_small against the library's host reference on every word and against sampling_exact's
    Philox4x32-10 in Python integers on the column sample"""
    import torch
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    n, qs = s.n, s.qs
    K = len(qs)
    for stacks in (1, big_count(n_power)):
        seed, stream_id = 0x1234567 + n_power, stacks
        cols = column_sample(stacks * n, 3 * n_power + stacks)
        out = filled(bits, stacks * K * n)
        with g.launch_log() as log:
            g.sample_uniform(out, qs, n_power, stacks, seed, stream_id)
        torch.cuda.synchronize()
        assert len(log.kernels) == 1
        got = g.to_host(out)
        assert np.array_equal(got, g.sample_reference_uniform(qs, n_power, stacks, seed, stream_id, bits=bits))
        view = got.reshape(stacks, K, n)
        for c in cols:
            st, j = divmod(int(c), n)
            for m, q in enumerate(qs):
                want, _ = uniform_word((st * K + m) * n + j, q, bits, seed, stream_id)
                assert int(view[st, m, j]) == want, (stacks, st, m, j)
        for distribution in (g.TERNARY, g.CBD21):
            small = filled(32, stacks * n)
            with g.launch_log() as log:
                g.sample_small(small, stacks, n_power, distribution, seed, stream_id)
            torch.cuda.synchronize()
            assert len(log.kernels) == 1
            got = g.to_host(small, signed=True)
            assert np.array_equal(got, g.sample_reference_small(stacks, n_power, distribution, seed, stream_id))
            assert all(int(got[c]) == small_word(int(c), distribution, seed, stream_id) for c in cols)


@sizes
def test_the_combine_kernels_every_word_against_python_integers(g, bits, n_power):
    """encrypt_public, encrypt_symmetric and generate_keys are lift_small, one forward transform and a per-column combine:
    the combine in Python integers (decrypt_exact.combine_public, keygen_exact.combine_encrypt / combine_keys) on what
    lift_small(to_ntt = true) returns for the same small values; operands of any words, the lift's edges planted"""
    import torch
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, qs, ks, M, D = s.L, s.n, s.qs, s.ks, s.M_p, s.D
    rng = np.random.default_rng(3000 * n_power + bits)
    sec_w = any_words(g, rng, bits, M * n, s.qp)
    sec, sec_h = device_words(g, sec_w), from_words(sec_w, (M, n))
    for count in (1, big_count(n_power)):
        small = planted_errors(rng, (3, count, n))
        d_small = small_device(small)
        lifted = filled(bits, 3 * count * L * n)
        ks.lift_small(d_small, lifted, 3 * count, False, True)
        pk_w, msg_w = any_words(g, rng, bits, 2 * L * n, qs), any_words(g, rng, bits, count * L * n, qs)
        pk, msg, out = device_words(g, pk_w), device_words(g, msg_w), filled(bits, 2 * count * L * n)
        ks.encrypt_public(pk, d_small, msg, out, count, zeros_bytes(ks.encrypt_public_scratch_bytes(count)))
        torch.cuda.synchronize()
        want = combine_public(qs, from_words(pk_w, (2, L, n)), host(g, lifted, (3, count, L, n)),
                              from_words(msg_w, (count, L, n)))
        assert np.array_equal(host(g, out, want.shape), want), ("encrypt_public", count)
        assert np.array_equal(g.to_host(pk), pk_w) and np.array_equal(g.to_host(msg), msg_w)

        a_w = any_words(g, rng, bits, count * L * n, qs)
        ct = filled(bits, 2 * count * L * n)
        ct[count * L * n:] = g.to_device(a_w)
        ks.encrypt_symmetric(sec, d_small[:count * n], msg, ct, count, zeros_bytes(ks.encrypt_scratch_bytes(count)))
        torch.cuda.synchronize()
        got = host(g, ct, (2, count, L, n))
        want = combine_encrypt(qs, L, host(g, lifted[:count * L * n], (count, L, n)), sec_h,
                               from_words(msg_w, (count, L, n)), from_words(a_w, (count, L, n)))
        assert np.array_equal(got[0], want), ("encrypt_symmetric", count)
        assert np.array_equal(got[1].reshape(-1), a_w.astype(object)), "a modified"
        assert np.array_equal(g.to_host(d_small, signed=True).reshape(small.shape), small)
    # generate_keys: keys D stacks of the full base; one key, and as many keys as make 2^17 columns (64 at the most)
    for keys in (1, min(64, max(2, big_count(n_power) // D))):
        errors = planted_errors(rng, (keys, D, n))
        d_err = small_device(errors)
        E = filled(bits, keys * D * M * n)
        ks.lift_small(d_err, E, keys * D, True, True)
        from_w = any_words(g, rng, bits, keys * M * n, s.qp)
        a_w = any_words(g, rng, bits, keys * D * M * n, s.qp).reshape(keys, D, M, n)
        dev = []
        for i in range(keys):
            k = filled(bits, D * 2 * M * n)
            k.view(D, 2, M, n)[:, 1] = g.to_device(a_w[i]).view(D, M, n)
            dev.append(k)
        ks.generate_keys(sec, device_words(g, from_w), d_err, dev, zeros_bytes(ks.keygen_scratch_bytes(keys)))
        torch.cuda.synchronize()
        want = combine_keys(s.qp, L, ALPHA, host(g, E, (keys, D, M, n)), sec_h, from_words(from_w, (keys, M, n)),
                            a_w.astype(object))
        for i, k in enumerate(dev):
            got = host(g, k, (D, 2, M, n))
            assert np.array_equal(got[:, 0], want[i]), ("generate_keys", keys, i)
            assert np.array_equal(got[:, 1], a_w[i].astype(object)), "a modified"
    assert np.array_equal(g.to_host(sec), sec_w), "s modified"


@pytest.mark.parametrize("bits", [64, 32])
def test_every_base_pointer_one_word_off_alignment(g, bits):
    """2^16, 3 stacks: the V = 1 path of every per-column kernel, where the tiles quadruple (u32) or double (u64): the
    words of the same calls on aligned copies; extend and scale_round against the host references, decode, phase,
    lift_small and scale_message against Python integers"""
    import torch
    n_power, stacks = 16, 3
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, qs, ks, bfv, M, Mb, Mp = s.L, s.n, s.qs, s.ks, s.bfv, s.M_p, s.M_b, s.M_p
    rng = np.random.default_rng(16 + bits)
    w = {"x": any_words(g, rng, bits, stacks * L * n, qs), "full": any_words(g, rng, bits, stacks * Mb * n, s.qb),
         "y": any_words(g, rng, bits, stacks * Mp * n, s.qp), "msg": any_words(g, rng, bits, stacks * n, [PLAIN]),
         "ct": any_words(g, rng, bits, 3 * stacks * L * n, qs), "s": any_words(g, rng, bits, M * n, s.qp),
         "pk": any_words(g, rng, bits, 2 * L * n, qs), "a": any_words(g, rng, bits, stacks * L * n, qs)}
    small = planted_errors(rng, (3, stacks, n))
    results = []
    for offset in (0, 1):
        d = {k: device_words(g, v, offset) for k, v in w.items()}
        d_small = small_device(small, offset)
        out = {"extend": filled(bits, stacks * Mb * n, offset), "scale_round": filled(bits, stacks * L * n, offset),
               "mod_down_add": filled(bits, stacks * L * n, offset), "scale_message": filled(bits, stacks * L * n, offset),
               "message": filled(bits, stacks * n, offset), "noise_max": filled(bits, stacks, offset),
               "message2": filled(bits, stacks * n, offset), "noise_max2": filled(bits, stacks, offset),
               "phase": filled(bits, stacks * L * n, offset), "lift_small": filled(bits, stacks * M * n, offset),
               "encrypt_public": filled(bits, 2 * stacks * L * n, offset),
               "encrypt_symmetric": filled(bits, 2 * stacks * L * n, offset),
               "generate_keys": filled(bits, s.D * 2 * M * n, offset),
               "uniform": filled(bits, stacks * L * n, offset), "small": filled(32, stacks * n, offset)}
        assert all(bool(t.data_ptr() % 16) == bool(offset) for t in list(d.values()) + list(out.values()) + [d_small])
        bfv.extend(d["x"], out["extend"], stacks)
        bfv.scale_round(d["full"], out["scale_round"], stacks)
        ks.mod_down_add(d["y"], d["a"], out["mod_down_add"], stacks)
        bfv.scale_message(d["msg"], out["scale_message"], stacks, False)
        bfv.decode(d["x"], out["message"], out["noise_max"], stacks)
        partials = filled(bits, bfv.decode_partials_bytes(stacks) // (bits // 8))
        with g.launch_log() as log:
            bfv.decode(d["x"], out["message2"], out["noise_max2"], stacks, partials=partials)
        assert log.kernels == ["bfv_decode", "bfv_decode_merge"]
        ks.phase(d["ct"], d["s"], out["phase"], stacks, 3, True, True)
        ks.lift_small(d_small, out["lift_small"], stacks, True, False)
        ks.encrypt_public(d["pk"], d_small, d["x"], out["encrypt_public"], stacks,
                          zeros_bytes(ks.encrypt_public_scratch_bytes(stacks)))
        out["encrypt_symmetric"][stacks * L * n:] = d["a"]
        ks.encrypt_symmetric(d["s"], d_small, d["x"], out["encrypt_symmetric"], stacks,
                             zeros_bytes(ks.encrypt_scratch_bytes(stacks)))
        # one key: s_from and the key's `a` planes are the words of y, the errors the first D small polynomials
        out["generate_keys"].view(s.D, 2, M, n)[:, 1] = d["y"][M * n:].view(s.D, M, n)
        ks.generate_keys(d["s"], d["y"], d_small, [out["generate_keys"]], zeros_bytes(ks.keygen_scratch_bytes(1)))
        g.sample_uniform(out["uniform"], qs, n_power, stacks, 99, 1)
        g.sample_small(out["small"], stacks, n_power, g.CBD21, 99, 2)
        torch.cuda.synchronize()
        for k, v in w.items():
            assert np.array_equal(g.to_host(d[k]), v), (k, "modified")
        results.append({k: v.clone() for k, v in out.items()})
    dt = g.np_dtype(bits)
    want = g.bfv_reference_extend(qs, s.qb[L:], w["x"], np.zeros(stacks * Mb * n, dtype=dt), n_power, stacks, bits)
    assert np.array_equal(g.to_host(results[1]["extend"]), want)
    want = g.bfv_reference_scale_round(qs, s.qb[L:], PLAIN, w["full"], np.zeros(stacks * L * n, dtype=dt), n_power,
                                       stacks, bits)
    assert np.array_equal(g.to_host(results[1]["scale_round"]), want)
    assert torch.equal(results[1]["noise_max2"], results[1]["noise_max"])
    assert torch.equal(results[1]["message2"], results[1]["message"])
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    # and the off-alignment words of the kernels without a host reference against Python integers
    off = results[1]
    m_want, n_want, _ = exact_decode(qs, PLAIN, from_words(w["x"], (stacks, L, n)), bits)
    assert np.array_equal(host(g, off["message"], m_want.shape), m_want), "decode"
    assert np.array_equal(host(g, off["noise_max"], (stacks,)), noise_max(n_want)), "noise_max"
    want = phase_words(qs, from_words(w["ct"], (3, stacks, L, n)), from_words(w["s"], (M, n)))
    assert np.array_equal(host(g, off["phase"], want.shape), want), "phase"
    want = lift(s.qp, small[0])  # the first `stacks` polynomials of small
    assert np.array_equal(host(g, off["lift_small"], want.shape), want), "lift_small"
    want = exact_scale_message(qs, PLAIN, from_words(w["msg"], (stacks, n)))
    assert np.array_equal(host(g, off["scale_message"], want.shape), want), "scale_message"


# ------------------------------------------------------------ 2. decode's noise maximum, every path of the reduction
# (bits, n_power, words off 16-byte alignment): the tile counts 128, 256, 64, 256 at 2^16, then 16, 64, 8, 32 and 128
DECODE_CASES = [(64, 16, 0), (64, 16, 1), (32, 16, 0), (32, 16, 1), (64, 13, 0), (64, 15, 0), (32, 13, 0), (32, 15, 0),
                (32, 15, 1)]
TILES = [128, 256, 64, 256, 16, 64, 8, 32, 128]


def decode_three_forms(g, bfv, bits, x, stacks, n, offset, tiles):
    """(message words, noise_max words) of the one-launch form, after checking that the two-launch form and the form
    without noise_max give the same words, the launch logs, and the guard words behind message_out"""
    import torch
    guard = 0x5A5A5A5A
    dx = object_words(g, x, bits, offset)
    assert bool(dx.data_ptr() % 16) == bool(offset)
    msg, worst = filled(bits, stacks * n + 16, offset, guard), filled(bits, stacks + 16, 0, guard)
    with g.launch_log() as log:
        bfv.decode(dx, msg[:-16], worst[:-16], stacks)
    torch.cuda.synchronize()
    assert log.kernels == ["bfv_decode"]
    msg2 = filled(bits, stacks * n + 16, offset, guard)
    with g.launch_log() as log:
        bfv.decode(dx, msg2[:-16], None, stacks)
    torch.cuda.synchronize()
    assert log.kernels == ["bfv_decode"]
    assert torch.equal(msg2, msg), "noise_max = None changes the messages or writes behind them"
    pbytes = bfv.decode_partials_bytes(stacks)
    assert pbytes >= stacks * tiles * (bits // 8)
    msg3, worst3 = filled(bits, stacks * n + 16, offset, guard), filled(bits, stacks + 16, 0, guard)
    part = filled(bits, pbytes // (bits // 8) + 16, 0, guard)
    with g.launch_log() as log:
        bfv.decode(dx, msg3[:-16], worst3[:-16], stacks, partials=part[:-16])
    torch.cuda.synchronize()
    assert log.kernels == ["bfv_decode", "bfv_decode_merge"]
    assert torch.equal(msg3, msg) and torch.equal(worst3, worst), "the two-launch form differs"
    assert (g.to_host(msg[stacks * n:]) == guard).all() and (g.to_host(worst[stacks:]) == guard).all()
    assert (g.to_host(part[-16:]) == guard).all()
    assert np.array_equal(host(g, dx, x.shape), x), "x modified"
    return host(g, msg[:stacks * n], (stacks, n)), host(g, worst[:stacks], (stacks,)), \
        host(g, part[:stacks * tiles], (stacks, tiles))


@pytest.mark.parametrize("bits,n_power,offset,tiles", [c + (t,) for c, t in zip(DECODE_CASES, TILES)],
                         ids=["u%d-2^%d-off%d" % c for c in DECODE_CASES])
def test_decode_noise_maximum_planted_in_a_chosen_tile_wave_and_lane(g, bits, n_power, offset, tiles):
    """x = round(Q m / t) + e with |e| below 8 noise words everywhere and one larger |e|, of either sign, per stack: tile
    0 lane 0; the last lane of the last tile; a lane of the last wave of a middle tile; a tile with index >= 64 where
    there is one (the second sweep of bfv_decode_merge's loop), the last lane of the first wave of tile 1 otherwise; one
    stack with nothing planted.  Messages, noise_max and the partial maxima of every tile against decrypt_exact"""
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, t, qs, Q, W = s.L, s.n, s.t, s.qs, s.Q, bits
    assert tiles == decode_tiles(bits, n_power, offset == 0)
    V = n // (256 * tiles)  # columns per lane
    unit = Q // (t << W)    # moving x by one unit moves the noise word by about one
    assert unit > 1 << 20
    rng = np.random.default_rng(n_power + bits + offset)
    stacks = 5
    x = noisy_phase(rng, Q, t, n, stacks, unit)

    def column(tile, lane, v=0):
        return (tile * 256 + lane) * V + v
    far = (tiles - 3, 70) if tiles > 64 else (1, 63)
    where = [(0, column(0, 0), 1000), (1, column(tiles - 1, 255, V - 1), -1100),
             (2, column(tiles // 2, 200), 1200), (4, column(*far), -1300)]  # stack 3 keeps its small noise
    assert far[0] >= 64 or tiles <= 64
    for stack, col, e in where:
        assert 0 <= col < n
        plant(x, Q, t, stack, col, e * unit)
    xl = limbs(x, qs)
    m_want, n_want, band = exact_decode(qs, t, xl, W)
    assert not band.any()
    worst_want = noise_max(n_want)
    assert len({int(v) for v in worst_want}) == stacks  # a maximum that leaked into a neighbour would show
    for stack, col, e in where:
        assert abs(int(n_want[stack, col])) == int(worst_want[stack]) and abs(abs(int(n_want[stack, col])) - abs(e)) < 16
        assert (int(n_want[stack, col]) > 0) == (e > 0)
    assert int(worst_want[3]) < 32
    msgs, worst, part = decode_three_forms(g, s.bfv, bits, xl, stacks, n, offset, tiles)
    assert np.array_equal(msgs, m_want)
    assert np.array_equal(worst, worst_want), (worst, worst_want)
    cols_per_tile = 256 * V
    part_want = np.array([[max(abs(int(v)) for v in n_want[k, i * cols_per_tile:(i + 1) * cols_per_tile])
                           for i in range(tiles)] for k in range(stacks)], dtype=object)
    assert np.array_equal(part, part_want), "a tile's partial maximum"
    print("bfv_decode_merge over %d tiles per stack at u%d 2^%d, %d words off alignment" % (tiles, bits, n_power, offset))


@pytest.mark.parametrize("bits", [64, 32])
def test_decode_the_most_negative_noise_word_and_the_band(g, bits):
    """2^16: one column whose noise word is -2^(W-1), whose magnitude 2^(W-1) does not fit the signed word, and one in the
    band [2^(W-1) - 3 L, 2^(W-1)), where the header allows round-half-up(t x / Q) or that value - 1 (mod t).  The columns
    are found by walking x in sixteenths of a unit around a rounding edge with decrypt_exact.exact_decode; the exact side says
    which of the two messages the definition gives, and the GPU gives that one"""
    n_power, stacks = 16, 2
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, t, qs, Q, W = s.L, s.n, s.t, s.qs, s.Q, bits
    half = 1 << (W - 1)
    unit = Q // (t << W)
    rng = np.random.default_rng(bits)
    k = int(rng.integers(1, t))
    edge = (Q * (2 * k + 1)) // (2 * t)
    cand = np.array([[(edge + j * (unit // 16)) % Q for j in range(-640, 641)]], dtype=object)
    _, c_noise, c_band = exact_decode(qs, t, limbs(cand, qs), W)
    lowest = [int(cand[0, j]) for j in range(cand.shape[1]) if int(c_noise[0, j]) == -half]
    inside = [int(cand[0, j]) for j in range(cand.shape[1]) if c_band[0, j]]
    assert lowest and inside, "the walk around the rounding edge found neither"
    x = noisy_phase(rng, Q, t, n, stacks, unit)
    tiles = decode_tiles(bits, n_power, True)
    col = [(tiles - 1) * (n // tiles) + 7, 65 * (n // tiles) + 3 if tiles > 65 else 5]
    x[0, col[0]], x[1, col[1]] = lowest[0], inside[len(inside) // 2]
    xl = limbs(x, qs)
    m_want, n_want, band = exact_decode(qs, t, xl, W)
    assert band.sum() == 1 and band[1, col[1]]
    assert int(n_want[0, col[0]]) == -half and half - 3 * L <= int(n_want[1, col[1]]) < half
    truth = [true_round(int(x[k_, c]), Q, t)[0] for k_, c in enumerate(col)]
    allowed = {truth[1], (truth[1] - 1) % t}
    given = int(m_want[1, col[1]])
    assert given in allowed
    print("u%d band column: round-half-up gives %d, the definition gives %s" %
          (bits, truth[1], "that value" if given == truth[1] else "that value - 1"))
    # at -2^(W-1) the noise is -1/2 within the band's 3 L / 2^W: the definition rounds up or down, both documented
    assert int(m_want[0, col[0]]) in (truth[0], (truth[0] - 1) % t)
    msgs, worst, _ = decode_three_forms(g, s.bfv, bits, xl, stacks, n, 0, tiles)
    assert np.array_equal(msgs, m_want)
    assert np.array_equal(worst, noise_max(n_want)) and int(worst[0]) == half and half - 3 * L <= int(worst[1]) < half


# ---------------------------------------------------- 3. the pipelines, word for word against their compositions
@rings
def test_multiply_equals_its_composition(g, bits, n_power, kind, L):
    """a product, the same with out given as x, and a squaring with y is x; coefficient form takes any words, NTT form
    residues"""
    s = Setup(g, bits, n_power, kind, L)
    n, t = s.n, s.t
    rng = np.random.default_rng(n_power + L + bits)
    deltas = {}
    for count in COUNTS:
        any_x, any_y = operands(g, rng, bits, s.qb, L, count, n)
        res_x, res_y = (reduced(g, v, s.qs, n, bits) for v in (any_x, any_y))
        keep = [v.clone() for v in (any_x, any_y, res_x, res_y)]
        scratch = bfv_scratch(s.bfv, count)
        words_in = 2 * count * L * n
        out, over = filled(bits, 3 * count * L * n), filled(bits, 3 * count * L * n)
        for input_ntt, output_ntt in FORMS:
            x, y = (res_x, res_y) if input_ntt else (any_x, any_y)
            what = (count, input_ntt, output_ntt)
            want = composition_multiply(g, s.st_b, L, t, x, y, count, input_ntt, output_ntt, n_power, bits)
            deltas[("product",) + what] = run_checked(
                s, p4_multiply(2, count, output_ntt),
                lambda i: s.bfvs[i].multiply(x, y, out, count, input_ntt, output_ntt, scratch), [out], [want], what)

            def over_x(i):
                over.fill_(-1)
                over[:words_in] = x
                s.bfvs[i].multiply(over, y, over, count, input_ntt, output_ntt, scratch)
            run_checked(s, p4_multiply(2, count, output_ntt), over_x, [over], [want], what + ("out is x",),
                        prefill=False)
            square = composition_multiply(g, s.st_b, L, t, x, x, count, input_ntt, output_ntt, n_power, bits)
            deltas[("squaring",) + what] = run_checked(
                s, p4_multiply(1, count, output_ntt),
                lambda i: s.bfvs[i].multiply(x, x, out, count, input_ntt, output_ntt, scratch), [out], [square],
                what + ("y is x",))
        unmodified((any_x, any_y, res_x, res_y), keep)
    report_p4(s, deltas)


def switching_key(s, rng):
    g = s.g
    return device_words(g, canonical_key(g, rng, s.bits, s.qp, s.D * 2 * s.M_p, s.n))


@rings
def test_multiply_relinearize_equals_its_composition(g, bits, n_power, kind, L):
    """also with out given as x, and with y is x"""
    s = Setup(g, bits, n_power, kind, L)
    n, t, D = s.n, s.t, s.D
    rng = np.random.default_rng(2 * n_power + L + bits)
    key = switching_key(s, rng)
    deltas = {}
    for count in COUNTS:
        any_x, any_y = operands(g, rng, bits, s.qb, L, count, n)
        res_x, res_y = (reduced(g, v, s.qs, n, bits) for v in (any_x, any_y))
        keep = [v.clone() for v in (any_x, any_y, res_x, res_y, key)]
        scratch, ks_scratch = bfv_scratch(s.bfv, count), relin_scratch(s.ks, count)
        out, over = filled(bits, 2 * count * L * n), filled(bits, 2 * count * L * n)
        for input_ntt, output_ntt in FORMS:
            x, y = (res_x, res_y) if input_ntt else (any_x, any_y)
            what = (count, input_ntt, output_ntt)
            want = composition_bfv(g, s.ks, s.st_b, s.st_p, t, x, y, key, count, input_ntt, output_ntt)
            eligible = p4_multiply_relinearize(2, D, count, output_ntt)
            deltas[("product",) + what] = run_checked(
                s, eligible, lambda i: s.bfvs[i].multiply_relinearize(x, y, s.kss[i], key, out, count, input_ntt,
                                                                      output_ntt, scratch, ks_scratch),
                [out], [want], what)

            def over_x(i):
                over.copy_(x)
                s.bfvs[i].multiply_relinearize(over, y, s.kss[i], key, over, count, input_ntt, output_ntt, scratch,
                                               ks_scratch)
            run_checked(s, eligible, over_x, [over], [want], what + ("out is x",), prefill=False)
            square = composition_bfv(g, s.ks, s.st_b, s.st_p, t, x, x, key, count, input_ntt, output_ntt)
            deltas[("squaring",) + what] = run_checked(
                s, p4_multiply_relinearize(1, D, count, output_ntt),
                lambda i: s.bfvs[i].multiply_relinearize(x, x, s.kss[i], key, out, count, input_ntt, output_ntt,
                                                         scratch, ks_scratch), [out], [square], what + ("y is x",))
        unmodified((any_x, any_y, res_x, res_y, key), keep)
    report_p4(s, deltas)


@rings
def test_multiply_sum_and_multiply_relinearize_sum_equal_their_compositions(g, bits, n_power, kind, L):
    """two terms that share their x: three distinct operands, 6 count polynomials per modulus in the forward transform;
    the auxiliary base is the smallest that holds two terms"""
    s = Setup(g, bits, n_power, kind, L, terms=2)
    n, t, D = s.n, s.t, s.D
    rng = np.random.default_rng(3 * n_power + L + bits)
    key = switching_key(s, rng)
    U = len({v for pair in SUM_PAIRS for v in pair})
    deltas = {}
    for count in COUNTS:
        anyw = [v for _ in range(2) for v in operands(g, rng, bits, s.qb, L, count, n)][:U]
        ops = {False: anyw, True: [reduced(g, v, s.qs, n, bits) for v in anyw]}
        keep = [v.clone() for v in ops[False] + ops[True] + [key]]
        scratch, ks_scratch = sum_scratch(s.bfv, count, U), relin_scratch(s.ks, count)
        assert scratch.numel() == max(256, s.bfv.sum_scratch_bytes(count, U))
        out3, out = filled(bits, 3 * count * L * n), filled(bits, 2 * count * L * n)
        for input_ntt, output_ntt in FORMS:
            xs, ys = [ops[input_ntt][a] for a, _ in SUM_PAIRS], [ops[input_ntt][b] for _, b in SUM_PAIRS]
            assert xs[0] is xs[1] and len({v.data_ptr() for v in xs + ys}) == U
            what = (count, input_ntt, output_ntt)
            want3 = composition_multiply_sum(g, s.st_b, L, t, xs, ys, count, input_ntt, output_ntt, n_power, bits)
            deltas[("multiply_sum",) + what] = run_checked(
                s, p4_multiply(U, count, output_ntt),
                lambda i: s.bfvs[i].multiply_sum(xs, ys, out3, count, input_ntt, output_ntt, scratch), [out3], [want3],
                ("multiply_sum",) + what)
            want = composition_bfv_sum(g, s.ks, s.st_b, s.st_p, t, xs, ys, key, count, input_ntt, output_ntt)
            deltas[("multiply_relinearize_sum",) + what] = run_checked(
                s, p4_multiply_relinearize(U, D, count, output_ntt),
                lambda i: s.bfvs[i].multiply_relinearize_sum(xs, ys, s.kss[i], key, out, count, input_ntt, output_ntt,
                                                             scratch, ks_scratch), [out], [want],
                ("multiply_relinearize_sum",) + what)
        unmodified(ops[False] + ops[True] + [key], keep)
    report_p4(s, deltas)


@rings
def test_relinearize_three_components_equals_its_composition(g, bits, n_power, kind, L):
    """the contiguous three-component layout; out separate and exactly c01"""
    s = Setup(g, bits, n_power, kind, L)
    n, D = s.n, s.D
    rng = np.random.default_rng(5 * n_power + L + bits)
    deltas = {}
    for count in COUNTS:
        low = 2 * count * L * n
        scratch = relin_scratch(s.ks, count)
        out = filled(bits, low)
        for input_ntt, output_ntt in FORMS:
            ct, key = relin3_operands(g, s.ks, s.st_p, rng, count, input_ntt)
            keep = [ct.clone(), key.clone()]
            what = (count, input_ntt, output_ntt)
            want = composition_relinearize(g, s.ks, s.st_p, ct[:low], ct[low:], key, count, input_ntt, output_ntt)
            eligible = p4_relinearize(D, count, output_ntt)
            deltas[what] = run_checked(
                s, eligible, lambda i: s.kss[i].relinearize(ct[:low], ct[low:], key, out, count, input_ntt, output_ntt,
                                                            scratch), [out], [want], what)
            unmodified((ct, key), keep)
            c01 = ct[:low].clone()

            def in_place(i):
                c01.copy_(ct[:low])
                s.kss[i].relinearize(c01, ct[low:], key, c01, count, input_ntt, output_ntt, scratch)
            run_checked(s, eligible, in_place, [c01], [want], what + ("out is c01",), prefill=False)
    report_p4(s, deltas)


def residue_ct(g, rng, bits, qs, polys, n):
    """polys stacks of the q-base, residues (both forms of decrypt and phase are defined on them)"""
    dt = g.np_dtype(bits)
    return np.concatenate([rng.integers(0, q, size=n, dtype=np.uint64).astype(dt) for _ in range(polys) for q in qs])


@rings
def test_decrypt_equals_phase_then_decode(g, bits, n_power, kind, L):
    """components 2 and 3, both input forms; decrypt decodes out of its own scratch.  The forward transform of the
    coefficient form runs over components count L polynomials"""
    s = Setup(g, bits, n_power, kind, L, t=PLAIN if (bits, kind) != (64, "narrow") else None)
    n = s.n
    assert usable(s.t, s.qs, bits)
    rng = np.random.default_rng(7 * n_power + L + bits)
    sec = device_words(g, residue_ct(g, rng, bits, s.qp, 1, n))
    deltas = {}
    for count in COUNTS:
        scratch = zeros_bytes(s.bfv.decrypt_scratch_bytes(count))
        assert s.bfv.decrypt_scratch_bytes(count) == -(-count * L * n * (bits // 8) // 256) * 256
        msg, worst = filled(bits, count * n), filled(bits, count)
        for components, input_ntt in itertools.product((2, 3), (True, False)):
            ct = device_words(g, residue_ct(g, rng, bits, s.qs, components * count, n))
            keep = [ct.clone(), sec.clone()]
            ks_scratch = zeros_bytes(s.ks.phase_scratch_bytes(count, components, input_ntt))
            ph, msg2, worst2 = filled(bits, count * L * n), filled(bits, count * n), filled(bits, count)
            s.ks.phase(ct, sec, ph, count, components, input_ntt, False, ks_scratch)
            s.bfv.decode(ph, msg2, worst2, count)
            what = (count, components, input_ntt)
            deltas[what] = run_checked(
                s, p4_groups(0 if input_ntt else components * count),
                lambda i: s.bfvs[i].decrypt(ct, s.kss[i], sec, msg, worst, count, components, input_ntt, scratch,
                                            None if input_ntt else ks_scratch), [msg, worst], [msg2, worst2], what)
            unmodified((ct, sec), keep)
    report_p4(s, deltas)


@rings
def test_generate_keys_and_encrypt_symmetric_equal_their_host_compositions(g, bits, n_power, kind, L):
    """keygen_exact on every word: the lift, the oracle's forward transform and the combine in Python integers.  Two
    keys in one call (2 D stacks of the full base, whole groups of four per modulus at D = 2); encrypt_symmetric at
    counts 1 to 4, with and without a message"""
    s = Setup(g, bits, n_power, kind, L)
    n, D, M, qs, ks = s.n, s.D, s.M_p, s.qs, s.ks
    cases = s.cases("p")
    rng = np.random.default_rng(11 * n_power + L + bits)
    sec_w = any_words(g, rng, bits, M * n, s.qp)
    sec, sec_h = device_words(g, sec_w), from_words(sec_w, (M, n))
    deltas = {}
    keys = 2
    errors = planted_errors(rng, (keys, D, n))
    from_w = any_words(g, rng, bits, keys * M * n, s.qp)
    a_w = any_words(g, rng, bits, keys * D * M * n, s.qp).reshape(keys, D, M, n)
    d_err, s_from = small_device(errors), device_words(g, from_w)
    dev = [filled(bits, D * 2 * M * n) for _ in range(keys)]
    want = exact_generate_keys(cases, L, ALPHA, sec_h, from_words(from_w, (keys, M, n)), errors, a_w.astype(object))
    wants = []
    for i in range(keys):
        w = np.stack([want[i], a_w[i].astype(object)], axis=1)  # [D][2][M][N]
        wants.append(object_words(g, w, bits))
    scratch = zeros_bytes(ks.keygen_scratch_bytes(keys))

    def gen(i):
        for k, a in zip(dev, a_w):
            k.view(D, 2, M, n)[:, 1] = g.to_device(a).view(D, M, n)
        s.kss[i].generate_keys(sec, s_from, d_err, dev, scratch)
    deltas["generate_keys"] = run_checked(s, p4_groups(keys * D), gen, dev, wants, "generate_keys")
    for count in COUNTS:
        err = planted_errors(rng, (count, n))
        d_e = small_device(err)
        a = any_words(g, rng, bits, count * L * n, qs)
        ct = filled(bits, 2 * count * L * n)
        scratch = zeros_bytes(ks.encrypt_scratch_bytes(count))
        for with_message in (True, False):
            msg_w = any_words(g, rng, bits, count * L * n, qs) if with_message else None
            msg = device_words(g, msg_w) if with_message else None
            c0 = exact_encrypt(cases, L, sec_h, err, from_words(msg_w, (count, L, n)) if with_message else None,
                               from_words(a, (count, L, n)))
            want_ct = object_words(g, np.stack([c0, from_words(a, (count, L, n))]), bits)

            def enc(i):
                ct[count * L * n:] = g.to_device(a)
                s.kss[i].encrypt_symmetric(sec, d_e, msg, ct, count, scratch)
            deltas[("encrypt_symmetric", count, with_message)] = run_checked(
                s, p4_groups(count), enc, [ct], [want_ct], ("encrypt_symmetric", count, with_message))
    assert np.array_equal(g.to_host(sec), sec_w) and np.array_equal(g.to_host(s_from), from_w)
    report_p4(s, deltas)


# ------------------------------------------------------------------- 4. exact integers at 2^16 on the widest primes
ENTRY_POINTS = ["multiply", "multiply_relinearize", "multiply_sum", "multiply_relinearize_sum", "relinearize",
                "generate_keys", "encrypt_symmetric", "encrypt_public", "phase", "decrypt"]
# the coefficients of multiply's result that lie in the rounding band of scale_round's first conversion, counted by
# bfv_exact.in_band on this test's seeded inputs: the words are compared there too -- the definition is word for word
BAND_HITS = {(64, True): 0, (64, False): 0, (32, True): 0, (32, False): 0}  # (bits, NTT form in and out)


def exact_operand_words(g, rng, bits, qs, count, n):
    """three operands T[2][count][L][N] of arbitrary words with 0, 2^W - 1, q - 1 and q planted, as numpy words: the
    host can draw the same ones without a device"""
    return [any_words(g, rng, bits, 2 * count * len(qs) * n, qs) for _ in range(3)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_against_exact_integers_at_2_16_on_the_widest_primes(g, entry, bits):
    """the compositions share kernels with what they check; here the expected words come from Python integers and the
    oracle's transforms alone.  count 1, operands of arbitrary words with the extremes planted (residues where the first
    step is a transform), NTT form in and out where the call has the forms"""
    import torch
    t0 = time.perf_counter()
    n_power, count, L = 16, 1, 3
    usable_t = entry in ("decrypt",)
    s = Setup(g, bits, n_power, "wide", L, t=PLAIN if usable_t else None,
              terms=2 if entry.endswith("sum") else 1)
    n, t, qs, D, M, bfv, ks = s.n, s.t, s.qs, s.D, s.M_p, s.bfv, s.ks
    assert max(s.qb).bit_length() == bits - 2
    cb, cp, cq = s.cases("b"), s.cases("p"), s.cases("q")
    rng = np.random.default_rng(16 + bits)
    host_s = 0.0

    def integers(tensor, shape):
        return from_words(g.to_host(tensor), shape)

    def compare(out, make_want, what):
        nonlocal host_s
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        want = make_want()
        host_s += time.perf_counter() - h0
        assert np.array_equal(integers(out, want.shape), want), what

    ct_shape = (2, count, L, n)
    if entry in ("multiply", "multiply_relinearize", "multiply_sum", "multiply_relinearize_sum"):
        raw = exact_operand_words(g, rng, bits, qs, count, n)
        ops = [reduced(g, device_words(g, w), qs, n, bits) for w in raw]
        hops = [integers(v, ct_shape) for v in ops]
        key = switching_key(s, rng)
        hkey = integers(key, (D, 2, M, n))
        ks_scratch = relin_scratch(ks, count)
        if entry == "multiply":
            # NTT form in and out on residues; coefficient form in and out on the arbitrary words themselves
            for ntt, xy in ((True, ops[:2]), (False, [device_words(g, w) for w in raw[:2]])):
                hxy = [integers(v, ct_shape) for v in xy]
                out = filled(bits, 3 * count * L * n)
                bfv.multiply(xy[0], xy[1], out, count, ntt, ntt, bfv_scratch(bfv, count))
                band = []

                def want():
                    w, b = exact_multiply(cb, L, t, bits, hxy[0], hxy[1], ntt, ntt)
                    band.append(int(b.sum()))
                    return w
                compare(out, want, (entry, ntt))
                print("band hits, NTT form %s: %d of %d coefficients" % (ntt, band[0], 3 * count * n))
                assert band[0] == BAND_HITS[(bits, ntt)], band
        elif entry == "multiply_relinearize":
            out = filled(bits, 2 * count * L * n)
            bfv.multiply_relinearize(ops[0], ops[1], ks, key, out, count, True, True, bfv_scratch(bfv, count), ks_scratch)
            compare(out, lambda: exact_bfv_multiply_relinearize(cb, cp, L, t, ALPHA, bits, hops[0], hops[1], hkey, True,
                                                                True), entry)
        else:
            xs, ys = [ops[a] for a, _ in SUM_PAIRS], [ops[b] for _, b in SUM_PAIRS]
            hx, hy = [hops[a] for a, _ in SUM_PAIRS], [hops[b] for _, b in SUM_PAIRS]
            scratch = sum_scratch(bfv, count, 3)
            if entry == "multiply_sum":
                out = filled(bits, 3 * count * L * n)
                bfv.multiply_sum(xs, ys, out, count, True, True, scratch)
                compare(out, lambda: exact_multiply_sum(cb, L, t, bits, hx, hy, True, True)[0], entry)
            else:
                out = filled(bits, 2 * count * L * n)
                bfv.multiply_relinearize_sum(xs, ys, ks, key, out, count, True, True, scratch, ks_scratch)
                compare(out, lambda: exact_multiply_relinearize_sum(cb, cp, L, t, ALPHA, bits, hx, hy, hkey, True, True),
                        entry)
    elif entry == "relinearize":
        low = 2 * count * L * n
        for input_ntt, output_ntt in ((True, True), (False, False)):
            ct, key = relin3_operands(g, ks, s.st_p, rng, count, input_ntt)
            h, hkey = integers(ct, (3, count, L, n)), integers(key, (D, 2, M, n))
            out = filled(bits, low)
            ks.relinearize(ct[:low], ct[low:], key, out, count, input_ntt, output_ntt, relin_scratch(ks, count))
            compare(out, lambda: exact_relinearize(cp, L, ALPHA, bits, h[:2], h[2], hkey, input_ntt, output_ntt),
                    (entry, input_ntt, output_ntt))
    elif entry in ("generate_keys", "encrypt_symmetric"):
        # s and s_from of any words; `a` sampled on the device: sampling_exact's Philox model on a column sample, the
        # library's host reference everywhere
        sec = device_words(g, any_words(g, rng, bits, M * n, s.qp))
        sec_h = integers(sec, (M, n))
        cols = column_sample(n, bits)
        if entry == "generate_keys":
            keys = 2
            errors = planted_errors(rng, (keys, D, n))
            s_from = device_words(g, any_words(g, rng, bits, keys * M * n, s.qp))
            dev = [filled(bits, D * 2 * M * n) for _ in range(keys)]
            for i, k in enumerate(dev):
                g.sample_uniform(k[M * n:], s.qp, n_power, D, 7, i, stack_stride_words=2 * M * n)
            a_h = np.stack([integers(k, (D, 2, M, n))[:, 1] for k in dev])
            for i in range(keys):
                ref = g.sample_reference_uniform(s.qp, n_power, D, 7, i, bits=bits)
                assert np.array_equal(a_h[i], from_words(ref, (D, M, n))), "a against the host reference"
                for d, m, j in itertools.product(range(D), range(M), cols):
                    assert int(a_h[i, d, m, j]) == uniform_word((d * M + m) * n + int(j), s.qp[m], bits, 7, i)[0], (i, d, m, j)
            ks.generate_keys(sec, s_from, small_device(errors), dev, zeros_bytes(ks.keygen_scratch_bytes(keys)))
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            want = exact_generate_keys(cp, L, ALPHA, sec_h, integers(s_from, (keys, M, n)), errors, a_h)
            host_s += time.perf_counter() - h0
            for i, k in enumerate(dev):
                got = integers(k, (D, 2, M, n))
                assert np.array_equal(got[:, 0], want[i]) and np.array_equal(got[:, 1], a_h[i]), i
        else:
            errors = planted_errors(rng, (count, n))
            msg = device_words(g, any_words(g, rng, bits, count * L * n, qs))
            ct = filled(bits, 2 * count * L * n)
            g.sample_uniform(ct[count * L * n:], qs, n_power, count, 8, 3)
            a_h = integers(ct, ct_shape)[1]
            ref = g.sample_reference_uniform(qs, n_power, count, 8, 3, bits=bits)
            assert np.array_equal(a_h, from_words(ref, (count, L, n))), "a against the host reference"
            for m, j in itertools.product(range(L), cols):
                assert int(a_h[0, m, j]) == uniform_word(m * n + int(j), qs[m], bits, 8, 3)[0], (m, j)
            ks.encrypt_symmetric(sec, small_device(errors), msg, ct, count, zeros_bytes(ks.encrypt_scratch_bytes(count)))
            hm = integers(msg, (count, L, n))
            compare(ct[:count * L * n], lambda: exact_encrypt(cp, L, sec_h, errors, hm, a_h), entry)
            assert np.array_equal(integers(ct, ct_shape)[1], a_h), "a modified"
    elif entry == "encrypt_public":
        small = planted_errors(rng, (3, count, n))
        pk = device_words(g, any_words(g, rng, bits, 2 * L * n, qs))
        msg = device_words(g, any_words(g, rng, bits, count * L * n, qs))
        out = filled(bits, 2 * count * L * n)
        ks.encrypt_public(pk, small_device(small), msg, out, count, zeros_bytes(ks.encrypt_public_scratch_bytes(count)))
        hpk, hm = integers(pk, (2, L, n)), integers(msg, (count, L, n))
        compare(out, lambda: exact_encrypt_public(cq, hpk, small, hm), entry)
    else:
        sec = device_words(g, any_words(g, rng, bits, M * n, s.qp))
        sec_h = integers(sec, (M, n))
        for components, input_ntt in ((3, True), (2, False)):
            raw = any_words(g, rng, bits, components * count * L * n, qs)
            ct_h = from_words(raw, (components, count, L, n))
            if not input_ntt:
                ct_h = ct_h % np.array(qs, dtype=object)[None, None, :, None]
            ct = object_words(g, ct_h, bits)
            ks_scratch = zeros_bytes(ks.phase_scratch_bytes(count, components, input_ntt))
            if entry == "phase":
                for output_ntt in (True, False):
                    out = filled(bits, count * L * n)
                    ks.phase(ct, sec, out, count, components, input_ntt, output_ntt, None if input_ntt else ks_scratch)
                    compare(out, lambda: exact_phase(cq, ct_h, sec_h, input_ntt, output_ntt),
                            (entry, components, input_ntt, output_ntt))
            else:
                msg, worst = filled(bits, count * n), filled(bits, count)
                bfv.decrypt(ct, ks, sec, msg, worst, count, components, input_ntt,
                            zeros_bytes(bfv.decrypt_scratch_bytes(count)), None if input_ntt else ks_scratch)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                m_want, n_want, _ = exact_decode(qs, t, exact_phase(cq, ct_h, sec_h, input_ntt, False), bits)
                host_s += time.perf_counter() - h0
                assert np.array_equal(integers(msg, (count, n)), m_want), (entry, components, input_ntt)
                assert np.array_equal(integers(worst, (count,)), noise_max(n_want)), (entry, components, input_ntt)
    print("exact integers, %s u%d: %.1f s, of which %.1f s the host reference"
          % (entry, bits, time.perf_counter() - t0, host_s))


# ------------------------------------------------------------- 5. the loop closes at parameters someone would use
class Loop:
    """everything made on the device, as tests/test_gpu_decrypt.py makes it at 2^12: a ternary secret, s^2, a
    relinearization key with cbd21 errors and a uniform `a`, a public key; buffers for one ciphertext pair"""

    def __init__(self, g, s, seed):
        bits, n_power, n, L, M, D, ks = s.bits, s.n_power, s.n, s.L, s.M_p, s.D, s.ks
        mods = [c.prm.modulus for c in s.cases("p")]
        self.s_small = filled(32, n)
        g.sample_small(self.s_small, 1, n_power, g.TERNARY, seed + 1, 0)
        self.s_ntt = filled(bits, M * n)
        ks.lift_small(self.s_small, self.s_ntt, 1, True, True)
        s_sq = filled(bits, M * n)
        for m in range(M):
            s_sq[m * n:(m + 1) * n] = g.operator_gpu(2, self.s_ntt[m * n:(m + 1) * n], self.s_ntt[m * n:(m + 1) * n],
                                                     mods[m])
        self.key = filled(bits, D * 2 * M * n)
        g.sample_uniform(self.key[M * n:], s.qp, n_power, D, seed + 2, 0, stack_stride_words=2 * M * n)
        key_err = filled(32, D * n)
        g.sample_small(key_err, D, n_power, g.CBD21, seed + 3, 0)
        ks.generate_keys(self.s_ntt, s_sq, key_err, [self.key], zeros_bytes(ks.keygen_scratch_bytes(1)))
        self.pk = filled(bits, 2 * L * n)
        g.sample_uniform(self.pk[L * n:], s.qs, n_power, 1, seed + 4, 0)
        e_pk = filled(32, n)
        g.sample_small(e_pk, 1, n_power, g.CBD21, seed + 5, 0)
        ks.encrypt_symmetric(self.s_ntt, e_pk, None, self.pk, 1, zeros_bytes(ks.encrypt_scratch_bytes(1)))


def sparse_message(rng, n, t):
    """64 seeded nonzero coefficients, coefficient 0 and N - 1 among them"""
    idx = np.concatenate([[0, n - 1], 1 + rng.choice(n - 2, size=62, replace=False)])
    val = rng.integers(1, t, size=64)
    m2 = np.zeros(n, dtype=np.int64)
    m2[idx] = val
    return idx, val, m2


@pytest.mark.parametrize("bits,n_power", [(64, 13), (64, 16), (32, 13), (32, 16)])
def test_the_loop_closes_at_parameters_someone_would_use(g, bits, n_power):
    """L = 3 on 60-bit (u64) and 30-bit (u32) primes, t = 65537.  A device-sampled ternary secret and cbd21 errors,
    generate_keys for s^2 -> s, encrypt_symmetric of scale_message(m1) (dense, uniform), encrypt_public of
    scale_message(m2) (64 nonzero coefficients), multiply_relinearize and decrypt with components 2, multiply and decrypt
    with components 3.  The expected plaintext is m1 m2 mod (t, X^N + 1) in Python integers: 64 shifted adds.

    Before a message is compared the phase of the result is worked out in Python integers
    (decrypt_exact.exact_phase on the device's ciphertext words) and its distance e from round(Q m / t) has to satisfy
    |e| t + t / 2 < Q / 2 - 3 L Q / 2^W: then decode's rounding is unambiguous (bfv_multiply.cuh, THE BAND) and a wrong
    message is a wrong message.  noise_max equals exact_decode's, and noise_budget_bits the header's formula for it"""
    import torch
    s = Setup(g, bits, n_power, "default", t=PLAIN)
    L, n, t, qs, Q, W, ks, bfv = s.L, s.n, s.t, s.qs, s.Q, bits, s.ks, s.bfv
    assert [q.bit_length() for q in qs] == ([60, 59, 58] if bits == 64 else [30, 29, 28])
    cq = s.cases("q")
    loop = Loop(g, s, 1000 * n_power + bits)
    rng = np.random.default_rng(n_power + bits)
    msgs = filled(bits, 2 * n, 0, 0)
    g.sample_uniform(msgs[:n], [t], n_power, 1, 77, 0)
    idx, val, m2 = sparse_message(rng, n, t)
    msgs[n:] = g.to_device(m2.astype(g.np_dtype(bits)))
    scaled = filled(bits, 2 * L * n)
    bfv.scale_message(msgs, scaled, 2, True)
    x, y = filled(bits, 2 * L * n), filled(bits, 2 * L * n)
    g.sample_uniform(x[L * n:], qs, n_power, 1, 78, 0)
    e1 = filled(32, n)
    g.sample_small(e1, 1, n_power, g.CBD21, 79, 0)
    ks.encrypt_symmetric(loop.s_ntt, e1, scaled[:L * n], x, 1, zeros_bytes(ks.encrypt_scratch_bytes(1)))
    small = filled(32, 3 * n)
    g.sample_small(small[:n], 1, n_power, g.TERNARY, 80, 0)
    g.sample_small(small[n:], 2, n_power, g.CBD21, 81, 0)
    ks.encrypt_public(loop.pk, small, scaled[L * n:], y, 1, zeros_bytes(ks.encrypt_public_scratch_bytes(1)))
    torch.cuda.synchronize()
    m1 = np.array([int(v) for v in g.to_host(msgs[:n])], dtype=object)
    assert max(m1) < t
    product = sparse_product(m1, idx, val, t)
    sec_h = host(g, loop.s_ntt, (s.M_p, n))
    cap = W - 1 - (3 * L).bit_length()
    d_scratch = zeros_bytes(bfv.decrypt_scratch_bytes(1))

    def check(ct, components, want, fresh, what):
        out_m, out_n = filled(bits, n), filled(bits, 1)
        bfv.decrypt(ct, ks, loop.s_ntt, out_m, out_n, 1, components, True, d_scratch, None)
        torch.cuda.synchronize()
        phase = exact_phase(cq, host(g, ct, (components, 1, L, n)), sec_h, True, False)
        X = crt(phase[0], qs)
        ideal = (Q * want + t // 2) // t  # scale_message's round(Q m / t)
        e = max(abs(int(v)) for v in centre((X - ideal) % Q, Q))
        margin = Q // 2 - (3 * L * Q >> W) - 1
        text = "%s u%d 2^%d: |e| = 2^%.1f of Q / (2 t) = 2^%.1f" % (what, bits, n_power, math.log2(e + 1),
                                                                    math.log2(Q / (2 * t)))
        assert e * t + t // 2 + 1 < margin, "the noise leaves decode's rounding ambiguous: " + text
        m_want, n_want, band = exact_decode(qs, t, phase, W)
        assert not band.any() and np.array_equal(m_want[0], want), text
        worst = int(g.to_host(out_n)[0])
        assert worst == int(noise_max(n_want)[0]), text
        budget = g.noise_budget_bits(worst, L, bits)
        assert budget == max(0, W - 1 - (worst + 3 * L).bit_length()), text
        if fresh:
            # Q / (2 t |e|) is far above 2^W here: the noise word is only decode's own slack (below 3 L; 2 to 4 on these
            # primes) and the budget reads as the documented cap W - 1 - bit_length(3 L), 59 bits at u64 and 27 at u32
            assert worst < 3 * L and budget == cap, ("a fresh ciphertext reads the documented cap", text, worst, budget,
                                                     cap)
        print(text + "; noise_max %d, budget %d bits (cap %d)" % (worst, budget, cap))
        assert np.array_equal(host(g, out_m, (n,)), want), text
        return budget

    check(x, 2, m1 % t, True, "fresh, symmetric")
    check(y, 2, np.array([int(v) for v in m2], dtype=object), True, "fresh, public key")
    prod = filled(bits, 2 * L * n)
    bfv.multiply_relinearize(x, y, ks, loop.key, prod, 1, True, True, bfv_scratch(bfv, 1), relin_scratch(ks, 1))
    check(prod, 2, product, False, "multiply_relinearize")
    prod3 = filled(bits, 3 * L * n)
    bfv.multiply(x, y, prod3, 1, True, True, bfv_scratch(bfv, 1))
    check(prod3, 3, product, False, "multiply, three components")


# --------------------------------------------------------------------- 6. memory, launches, graph, all at 2^16
def pipeline_calls(s, bfv, ks, data, outs, scr):
    """every call of sections 3 and 5 on one plan pair; outs / scr: dicts of tensors by call"""
    count = data["count"]
    x, y, z, key = data["x"], data["y"], data["z"], data["key"]
    bfv.multiply(x, y, outs["multiply"], count, True, True, scr["multiply"])
    bfv.multiply_relinearize(x, y, ks, key, outs["multiply_relinearize"], count, True, True, scr["multiply"],
                             scr["relin"])
    bfv.multiply_sum([x, x], [y, z], outs["multiply_sum"], count, True, True, scr["sum"])
    bfv.multiply_relinearize_sum([x, x], [y, z], ks, key, outs["multiply_relinearize_sum"], count, True, True,
                                 scr["sum"], scr["relin"])
    low = 2 * count * s.L * s.n
    ks.relinearize(outs["multiply"][:low], outs["multiply"][low:], key, outs["relinearize"], count, True, True,
                   scr["relin"])
    ks.generate_keys(data["s"], data["s_from"], data["key_err"], [outs["generate_keys"]], scr["keygen"])
    bfv.scale_message(data["msg"], outs["scale_message"], count, True)
    ks.encrypt_symmetric(data["s"], data["small"][:count * s.n], outs["scale_message"], outs["encrypt_symmetric"], count,
                         scr["encrypt"])
    ks.encrypt_public(data["pk"], data["small"], outs["scale_message"], outs["encrypt_public"], count,
                      scr["encrypt_public"])
    ks.phase(outs["multiply"], data["s"], outs["phase"], count, 3, False, False, scr["phase"])
    bfv.decode(outs["phase"], outs["decode_m"], outs["decode_n"], count, partials=scr["partials"])
    bfv.decrypt(outs["multiply_relinearize"], ks, data["s"], outs["decrypt_m"], outs["decrypt_n"], count, 2, False,
                scr["decrypt"], scr["phase"])


@pytest.mark.parametrize("bits", [64, 32])
def test_caller_owned_workspaces_and_exact_scratches_between_guards(g, bits):
    """both plans in workspaces of exactly workspace_bytes() and every scratch of exactly its size carved out of 0xA5:
    the words of plans that own their workspace and of generous scratches, no guard byte touched, no device memory
    allocated by any call"""
    import torch
    n_power, count, L = 16, 2, 3
    s = Setup(g, bits, n_power, "default", L, t=PLAIN, terms=2)
    n, M, D, qs = s.n, s.M_p, s.D, s.qs
    big_b, ws_b = guarded(g.BfvMultiplyPlan.workspace_bytes(L, s.K_b, n_power, bits))
    big_p, ws_p = guarded(g.KeySwitchPlan.workspace_bytes(L, K_P, ALPHA, n_power, bits))
    bfv = make_bfv_plan(g, s.st_b, L, s.t, n_power, bits, workspace=ws_b)
    ks = make_plan(g, s.st_p, L, ALPHA, n_power, bits, workspace=ws_p)
    assert not bfv.owns_workspace and not ks.owns_workspace and s.bfv.owns_workspace and s.ks.owns_workspace
    rng = np.random.default_rng(6 + bits)
    ops = [reduced(g, v, qs, n, bits) for _ in range(2) for v in operands(g, rng, bits, s.qb, L, count, n)]
    data = dict(count=count, x=ops[0], y=ops[1], z=ops[2], key=switching_key(s, rng),
                s=device_words(g, residue_ct(g, rng, bits, s.qp, 1, n)),
                s_from=device_words(g, residue_ct(g, rng, bits, s.qp, 1, n)),
                key_err=small_device(planted_errors(rng, (D, n))), small=small_device(planted_errors(rng, (3, count, n))),
                msg=device_words(g, any_words(g, rng, bits, count * n, [PLAIN])),
                pk=device_words(g, residue_ct(g, rng, bits, qs, 2, n)))
    ct3, ct2 = 3 * count * L * n, 2 * count * L * n
    sizes_ = {"multiply": ct3, "multiply_relinearize": ct2, "multiply_sum": ct3, "multiply_relinearize_sum": ct2,
              "relinearize": ct2, "generate_keys": D * 2 * M * n, "scale_message": count * L * n,
              "encrypt_symmetric": ct2, "encrypt_public": ct2, "phase": count * L * n, "decode_m": count * n,
              "decode_n": count, "decrypt_m": count * n, "decrypt_n": count}
    sbytes = {"multiply": bfv.scratch_bytes(count), "sum": bfv.sum_scratch_bytes(count, 3),
              "relin": ks.scratch_bytes(count, 2), "keygen": ks.keygen_scratch_bytes(1),
              "encrypt": ks.encrypt_scratch_bytes(count), "encrypt_public": ks.encrypt_public_scratch_bytes(count),
              "phase": ks.phase_scratch_bytes(count, 3, False), "partials": bfv.decode_partials_bytes(count),
              "decrypt": bfv.decrypt_scratch_bytes(count)}
    assert ks.phase_scratch_bytes(count, 2, False) <= sbytes["phase"]

    def views(make):
        out = {k: make(v) for k, v in sbytes.items()}
        return out

    def typed(d):
        r = dict(d)
        r["partials"] = d["partials"].view(tdtype(bits))
        return r

    def fresh_outs():
        outs = {k: filled(bits, v) for k, v in sizes_.items()}
        for o in (outs["generate_keys"], outs["encrypt_symmetric"]):  # the `a` planes are inputs
            o.fill_(12345)
        return outs
    want = fresh_outs()
    pipeline_calls(s, s.bfv, s.ks, data, want, typed(views(lambda v: zeros_bytes(2 * v + 4096))))
    torch.cuda.synchronize()
    got = fresh_outs()
    bigs = views(lambda v: guarded(max(256, v)))
    scr = typed({k: view for k, (_, view) in bigs.items()})
    torch.cuda.synchronize()
    before, allocs = torch.cuda.memory_allocated(), g.alloc_count()
    pipeline_calls(s, bfv, ks, data, got, scr)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and g.alloc_count() == allocs
    for k in sizes_:
        assert torch.equal(got[k], want[k]), k
    assert guards_intact(big_b), "BfvMultiplyPlan workspace guard"
    assert guards_intact(big_p), "KeySwitchPlan workspace guard"
    for k, (big, _) in bigs.items():
        assert guards_intact(big), k


@pytest.mark.parametrize("bits,n_power", [(64, 15), (64, 16), (32, 16)])
def test_multiply_and_decrypt_launch_the_stand_alone_transforms_around_their_own_kernels(g, bits, n_power):
    """multiply's launch log is that of four stand-alone NTTPlans of the same batches with bfv_extend per operand,
    bfv_tensor and bfv_scale_round where "What runs" puts them; u64 from 2^15 and u32 at 2^16 every transform is two
    sweeps (README): at least two kernels per stage.  The same for decrypt: the q-base forward transform of the
    coefficient form, decrypt_phase, the q-base inverse, bfv_decode"""
    import torch
    L, count = 3, 2
    s = Setup(g, bits, n_power, "default", L, t=PLAIN)
    n, Mb, bfv, ks = s.n, s.M_b, s.bfv, s.ks
    buf = torch.zeros(4 * count * Mb * n, dtype=tdtype(bits), device="cuda:0")
    stages = {}
    for name, st, table, kind, mods, batch in (
            ("inv_q", s.st_b, "inv", g.INVERSE, s.cases("q"), 2 * count * L),
            ("fwd_full", s.st_b, "fwd", g.FORWARD, s.cases("b"), 4 * count * Mb),
            ("fwd_full_square", s.st_b, "fwd", g.FORWARD, s.cases("b"), 2 * count * Mb),
            ("inv_full", s.st_b, "inv", g.INVERSE, s.cases("b"), 3 * count * Mb),
            ("fwd_q", s.st_b, "fwd", g.FORWARD, s.cases("q"), 3 * count * L),
            ("phase_fwd", s.st_p, "fwd", g.FORWARD, s.cases("q"), 3 * count * L),
            ("phase_inv", s.st_p, "inv", g.INVERSE, s.cases("q"), count * L)):
        mc = len(mods)
        alone = g.NTTPlan(st[table], [c.prm.modulus for c in mods], n_power, g.X_N_plus, kind, st["n_inv"][:mc],
                          batch_hint=1024)
        with g.launch_log() as log:
            alone.execute(buf, buf, batch)
        torch.cuda.synchronize()
        alone.close()
        stages[name] = log.kernels
        assert len(log.kernels) >= 2, (name, log.kernels)
    x, y = (torch.zeros(2 * count * L * n, dtype=tdtype(bits), device="cuda:0") for _ in range(2))
    out, scratch = filled(bits, 3 * count * L * n), bfv_scratch(bfv, count)
    for input_ntt, output_ntt in FORMS:
        head, tail = (stages["inv_q"] if input_ntt else []), (stages["fwd_q"] if output_ntt else [])
        with g.launch_log() as log:
            bfv.multiply(x, y, out, count, input_ntt, output_ntt, scratch)
        want = head + ["bfv_extend"] + head + ["bfv_extend"] + stages["fwd_full"] + ["bfv_tensor"] + \
            stages["inv_full"] + ["bfv_scale_round"] + tail
        assert log.kernels == want, (log.kernels, want)
        with g.launch_log() as log:
            bfv.multiply(x, x, out, count, input_ntt, output_ntt, scratch)
        want = head + ["bfv_extend"] + stages["fwd_full_square"] + ["bfv_tensor"] + stages["inv_full"] + \
            ["bfv_scale_round"] + tail
        assert log.kernels == want, (log.kernels, want)
    sec = torch.zeros(s.M_p * n, dtype=tdtype(bits), device="cuda:0")
    msg, worst = filled(bits, count * n), filled(bits, count)
    d_scratch = zeros_bytes(bfv.decrypt_scratch_bytes(count))
    k_scratch = zeros_bytes(ks.phase_scratch_bytes(count, 3, False))
    for input_ntt in (True, False):
        with g.launch_log() as log:
            bfv.decrypt(out, ks, sec, msg, worst, count, 3, input_ntt, d_scratch, None if input_ntt else k_scratch)
        want = ([] if input_ntt else stages["phase_fwd"]) + ["decrypt_phase"] + stages["phase_inv"] + ["bfv_decode"]
        assert log.kernels == want, (log.kernels, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [64, 32])
def test_encrypt_multiply_relinearize_decrypt_in_one_graph_replayed_with_new_messages(g, bits):
    """2^16, one side stream, a linear capture of scale_message -> encrypt_symmetric (twice) -> multiply_relinearize ->
    decrypt; replayed twice with new messages written into the captured buffers: the decrypted words are
    m1 m2 mod (t, X^N + 1) in Python integers and noise_max equals exact_decode's on the replayed ciphertext"""
    import torch
    n_power, L = 16, 3
    s = Setup(g, bits, n_power, "default", L, t=PLAIN)
    n, t, qs, ks, bfv = s.n, s.t, s.qs, s.ks, s.bfv
    loop = Loop(g, s, 5000 + bits)
    msgs, scaled = filled(bits, 2 * n, 0, 0), filled(bits, 2 * L * n)
    cts = filled(bits, 2 * 2 * L * n).view(2, -1)
    errs = filled(32, 2 * n)
    g.sample_small(errs, 2, n_power, g.CBD21, 31, 0)
    prod, out_m, out_n = filled(bits, 2 * L * n), filled(bits, n), filled(bits, 1)
    e_scratch, b_scratch, k_scratch = (zeros_bytes(ks.encrypt_scratch_bytes(1)), bfv_scratch(bfv, 1),
                                       relin_scratch(ks, 1))
    d_scratch = zeros_bytes(bfv.decrypt_scratch_bytes(1))
    a = [filled(bits, L * n) for _ in range(2)]
    for i in range(2):
        g.sample_uniform(a[i], qs, n_power, 1, 32, i)

    def run(stream):
        bfv.scale_message(msgs, scaled, 2, True, stream=stream)
        for i in range(2):
            ks.encrypt_symmetric(loop.s_ntt, errs[i * n:(i + 1) * n], scaled[i * L * n:(i + 1) * L * n], cts[i], 1,
                                 e_scratch, stream=stream)
        bfv.multiply_relinearize(cts[0], cts[1], ks, loop.key, prod, 1, True, True, b_scratch, k_scratch, stream=stream)
        bfv.decrypt(prod, ks, loop.s_ntt, out_m, out_n, 1, 2, True, d_scratch, None, stream=stream)

    def new_messages(seed):
        rng = np.random.default_rng(seed)
        idx, val, m2 = sparse_message(rng, n, t)
        m1 = rng.integers(0, t, size=n)
        msgs[:n] = g.to_device(m1.astype(g.np_dtype(bits)))
        msgs[n:] = g.to_device(m2.astype(g.np_dtype(bits)))
        for i in range(2):  # encrypt_symmetric reads `a` from its output: put it back
            cts[i][L * n:] = a[i]
        return sparse_product(m1, idx, val, t)
    new_messages(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # eager warm-up on the capture stream
        run(side)
    side.synchronize()
    allocs = g.alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(side)
    sec_h = host(g, loop.s_ntt, (s.M_p, n))
    for seed in (1, 2):
        want = new_messages(seed)
        out_m.fill_(-1), out_n.fill_(-1), prod.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(g, out_m, (n,)), want), seed
        phase = exact_phase(s.cases("q"), host(g, prod, (2, 1, L, n)), sec_h, True, False)
        m_want, n_want, band = exact_decode(qs, t, phase, bits)
        assert not band.any() and np.array_equal(m_want[0], want), seed
        assert int(g.to_host(out_n)[0]) == int(noise_max(n_want)[0]), seed
    assert g.alloc_count() == allocs
