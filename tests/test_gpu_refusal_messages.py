"""The words and the precedence of every refusal of the pipeline calls of KeySwitchPlan, BfvMultiplyPlan and
BfvBatchEncoder (csrc/rns_call.hpp is the unit their checks share).  The calls go through the C interface with raw
addresses: the Python wrapper has size and null checks of its own, which would answer first.  Per entry point a table of
(what is wrong, arguments, expected message); the message is compared word for word and the launch log must be empty.
An expected message of None is an alias the call allows ("out may be exactly x"): it is accepted and launches.  Every
address lies in one zeroed arena, 64 KiB apart unless a case says otherwise, so no call reads or writes outside it.
n_power = 4, L = 3, K = 2, alpha = 2, count = 2, rescale_limbs = 1, both word widths."""
import ctypes

import pytest

from bfv_utils import aux_count
from bfv_utils import make_plan as make_bfv_plan
from encode_utils import Encoder, plain_for_ring
from hoisted_utils import make_plan, ring

pytestmark = pytest.mark.gpu

N_POWER, L, K, ALPHA, COUNT, R = 4, 3, 2, 2, 2, 1
M, N = L + K, 1 << N_POWER
SLOT = 1 << 16

NULL = "null pointer argument"
ALIGN = "The scratch is not 256-byte aligned!"
OPERAND = "out or the scratch overlaps an operand!"
S_OUT = "The scratch overlaps out!"
S_OP = "The scratch overlaps an operand!"
TABLES = "The plan was built without transform tables!"
RESCALE = "The plan was built without rescale_limbs!"
BAD_COUNT = "Invalid count!"
ODD = "Invalid Galois element (must be odd)!"
MATCH = "The key-switching plan does not match!"


def align(b):
    return (b + 255) // 256 * 256


class Env:
    def __init__(self, g, bits):
        import torch
        self.g, self.bits, self.lib, self.T, self.S = g, bits, g.load_library(), bits // 8, "u%d" % bits
        self.ring = ring(g, bits, N_POWER)  # 8 primes
        st = self.ring.sub(list(range(M)))
        self.plan = make_plan(g, st, L, ALPHA, N_POWER, bits, rescale_limbs=R)
        self.plain = make_plan(g, st, L, ALPHA, N_POWER, bits)  # R = 0
        self.bare = g.KeySwitchPlan(st["moduli"][:L], st["moduli"][L:], ALPHA, N_POWER, bits=bits, rescale_limbs=R)
        self.wide_keys = make_plan(g, st, L, ALPHA, N_POWER, bits, key_mod_count=M + 1)
        self.other = make_plan(g, st, L - 1, ALPHA, N_POWER, bits)  # another q-base
        self.D = self.plan.digits
        t = plain_for_ring(N_POWER)
        kb = aux_count(self.ring.moduli, L, t[0], N)
        kb = min(kb + 1, len(self.ring.moduli) - L)  # room for the terms of a sum
        self.bfv = make_bfv_plan(g, self.ring.sub(list(range(L + kb))), L, t[0], N_POWER, bits)
        self.encoder = Encoder(g, bits, N_POWER, t)
        self.arena = torch.zeros(64 * SLOT + 256, dtype=torch.uint8, device="cuda:0")
        self.next = align(self.arena.data_ptr())
        self.end = self.arena.data_ptr() + self.arena.numel()
        self.names = {}
        poly = COUNT * N * self.T
        self.POLY, self.A, self.CT1, self.KEY = poly, poly * M * self.D, poly * L, self.D * 2 * M * N * self.T
        self.c_coeff = align(self.A)  # the layout of scratch_bytes(count, components)
        self.inner_out = self.c_coeff + align(self.CT1)
        self.OFF = 8 * self.T  # "8 words off"

    def b(self, name):
        """the address of a named region: 64 KiB, 256-byte aligned, zeroed, apart from every other"""
        if name not in self.names:
            self.names[name] = self.next
            self.next += SLOT
            assert self.next <= self.end
        return self.names[name]

    def word(self, v):
        return (ctypes.c_uint32 if self.bits == 32 else ctypes.c_uint64)(v)


_envs = {}


@pytest.fixture(params=[64, 32])
def env(pkg, request):
    pkg.load_library()
    if request.param not in _envs:
        _envs[request.param] = Env(pkg, request.param)
    return _envs[request.param]


def P(address):
    return None if address is None else ctypes.c_void_p(address)


def ptrs(*addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


def u32s(*values):
    return (ctypes.c_uint32 * len(values))(*values)


def walk(env, name, cases):
    """cases: (what, arguments after the plan, expected message or None[, the plan if not env.plan])"""
    fn = getattr(env.lib, "gpuntt_%s_%s" % (name, env.S))
    wrong = []
    for what, args, want, *other in cases:
        plan = other[0] if other else env.plan
        args = [P(a) if isinstance(a, int) and a >= SLOT else a for a in args]  # an int that large is an address
        with env.g.launch_log() as log:
            rc = fn(plan._h, *args, None)
        got = env.lib.gpuntt_last_error().decode() if rc else None
        print("%s %s: %s -> %r %s" % (name, env.S, what, got, log.kernels[:2]))
        ok = (got is None and log.kernels) if want is None else (got == want and log.kernels == [])
        if not ok:
            wrong.append((what, want, got, log.kernels))
    import torch
    torch.cuda.synchronize()
    assert not wrong, wrong


def test_decompose(env):
    e = env
    c, a, s = e.b("c_in"), e.b("a"), e.b("scratch")
    walk(e, "keyswitch_plan_decompose", [
        ("no tables", (c, a, COUNT, 1, s), TABLES, e.bare),
        ("negative count", (c, a, -1, 1, s), BAD_COUNT),
        ("null c_in", (None, a, COUNT, 1, s), NULL),
        ("null scratch, NTT input", (c, a, COUNT, 1, None), NULL),
        ("a 8 words into c_in", (c, c + e.OFF, COUNT, 0, None), "ModUp input and output overlap!"),
        ("c_in in the scratch's coefficient region", (s + e.c_coeff, a, COUNT, 1, s), S_OP),
        ("a in the scratch's coefficient region", (c, s + e.c_coeff, COUNT, 1, s), S_OP),
        ("negative count and null scratch", (c, a, -1, 1, None), BAD_COUNT),
        ("a over c_in and over the scratch", (s + e.c_coeff, s + e.c_coeff + e.OFF, COUNT, 1, s),
         "ModUp input and output overlap!"),
    ])


def test_switch_digits(env):
    e = env
    a, key, out, s = e.b("a"), e.b("key"), e.b("out"), e.b("scratch")
    walk(e, "keyswitch_plan_switch_digits", [
        ("no tables", (a, key, out, COUNT, 2, 0, s), TABLES, e.bare),
        ("negative count", (a, key, out, -1, 2, 0, s), BAD_COUNT),
        ("no components", (a, key, out, COUNT, 0, 0, s), "Invalid components!"),
        ("null scratch", (a, key, out, COUNT, 2, 0, None), NULL),
        ("out in the scratch's accumulators", (a, key, s + e.inner_out, COUNT, 2, 0, s), S_OUT),
        ("negative count and no components", (a, key, out, -1, 0, 0, s), BAD_COUNT),
    ])


def test_apply(env):
    e = env
    c, key, out, s = e.b("c_in"), e.b("key"), e.b("out"), e.b("scratch")
    walk(e, "keyswitch_plan_apply", [
        ("no tables", (c, key, out, COUNT, 2, 0, 0, s), TABLES, e.bare),
        ("negative count", (c, key, out, -1, 2, 0, 0, s), BAD_COUNT),
        ("null key", (c, None, out, COUNT, 2, 0, 0, s), NULL),
        ("c_in is the scratch", (s, key, out, COUNT, 2, 0, 0, s), S_OP),
        ("out in the scratch", (c, key, s + 256, COUNT, 2, 0, 0, s), S_OP),
    ])


def test_mod_down_add(env):
    e = env
    x, addend, out = e.b("x"), e.b("addend"), e.b("out")
    walk(e, "keyswitch_plan_mod_down_add", [
        ("negative stacks", (x, addend, out, -1), "Invalid stacks!"),
        ("null addend", (x, None, out, COUNT), NULL),
        ("addend exactly out", (x, out, out, COUNT), None),
        ("addend 8 words into out", (x, out + e.OFF, out, COUNT), "The addend overlaps an operand!"),
        ("addend inside x", (x, x + e.OFF, out, COUNT), "The addend overlaps an operand!"),
        ("out inside x", (x, addend, x + e.OFF, COUNT), "ModDown input and output overlap!"),
        ("out inside x and the addend too", (x, x + 2 * e.OFF, x + e.OFF, COUNT), "ModDown input and output overlap!"),
    ])


def test_rescale(env):
    e = env
    x, out, s = e.b("x"), e.b("out"), e.b("scratch")
    walk(e, "keyswitch_plan_rescale", [
        ("no rescale_limbs", (x, out, COUNT, 1, s), RESCALE, e.plain),
        ("no tables", (x, out, COUNT, 1, s), TABLES, e.bare),
        ("negative stacks", (x, out, -1, 1, s), "Invalid stacks!"),
        ("null x", (None, out, COUNT, 1, s), NULL),
        ("null scratch, NTT form", (x, out, COUNT, 1, None), NULL),
        ("misaligned scratch", (x, out, COUNT, 1, s + 8), ALIGN),
        ("out inside x", (x, x + e.OFF, COUNT, 1, s), "ModDown input and output overlap!"),
        ("the scratch inside x", (x, out, COUNT, 1, x + 256), S_OP),
        ("the scratch is out", (x, out, COUNT, 1, out), S_OUT),
        ("negative stacks and null scratch", (x, out, -1, 1, None), "Invalid stacks!"),
        ("misaligned scratch inside x", (x, out, COUNT, 1, x + 8), ALIGN),
        ("the scratch over x (at 32 bits over out too), out behind x", (x, x + e.CT1, COUNT, 1, x + 256), S_OP),
    ])


def hoisted_cases(e, sum_form):
    a, c0, out, s, k0, k1, w = (e.b(n) for n in ("a", "c0", "out", "scratch", "key0", "key1", "weight"))

    def args(a=a, c0=c0, keys=(k0, k1), elts=(3, 5), weights=None, G=2, out=out, count=COUNT, scratch=s):
        mid = (None if weights is None else ptrs(*weights),) if sum_form else ()
        return (a, c0, None if keys is None else ptrs(*keys), None if elts is None else u32s(*elts)) + mid + \
            (G, out, count, 1, scratch)

    cases = [
        ("no tables", args(), TABLES, e.bare),
        ("negative count", args(count=-1), BAD_COUNT),
        ("no elements", args(G=0), "Invalid galois_count!"),
        ("65 elements", args(G=65), "Invalid galois_count!"),
        ("null a", args(a=None), NULL),
        ("null elements", args(elts=None), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("an even element", args(elts=(3, 4)), ODD),
        ("an element even modulo 2 N", args(elts=(3, 36)), ODD),
        ("a null key", args(keys=(k0, None)), NULL),
        ("out 8 words into a", args(out=a + e.OFF), OPERAND),
        ("a key in the scratch", args(keys=(k0, s + 512)), OPERAND),
        ("c0 8 words into out", args(c0=out + e.OFF), OPERAND),
        ("null c0, out is the scratch", args(c0=None, out=s), S_OUT),
        ("negative count and null a", args(count=-1, a=None), BAD_COUNT),
        ("null a and a misaligned scratch", args(a=None, scratch=s + 8), NULL),
        ("a misaligned scratch and an even element", args(scratch=s + 8, elts=(4, 5)), ALIGN),
        ("a misaligned scratch and a null key", args(scratch=s + 8, keys=(None, k1)), ALIGN),
        ("an even element with a null key", args(elts=(4, 5), keys=(None, k1)), ODD),
        ("a null key before an even element", args(elts=(3, 4), keys=(None, k1)), NULL),
        ("an operand overlap and out is the scratch", args(a=s + 256, out=s), OPERAND),
    ]
    if sum_form:
        cases += [
            ("null weights, out is the scratch", args(weights=None, out=s), S_OUT),
            ("one null weight, the other 8 words into out", args(weights=(None, out + e.OFF)), OPERAND),
            ("a weight in the scratch", args(weights=(w, s + 256)), OPERAND),
        ]
    return cases


def test_rotate_hoisted(env):
    walk(env, "keyswitch_plan_rotate_hoisted", hoisted_cases(env, False))


def test_rotate_hoisted_sum(env):
    cases = hoisted_cases(env, True)
    walk(env, "keyswitch_plan_rotate_hoisted_sum", cases)
    walk(env, "keyswitch_plan_rotate_hoisted_sum_rescale",
         [("no rescale_limbs", cases[0][1], RESCALE, env.plain), ("no tables", cases[0][1], TABLES, env.bare)] + cases[1:])


def test_linear_transform_bsgs(env):
    e = env
    a, c0, c1, out, s = (e.b(n) for n in ("a", "c0", "c1", "out", "scratch"))
    k = [e.b("key%d" % i) for i in range(4)]
    w = [e.b("weight%d" % i) for i in range(4)]
    steps = "Invalid baby or giant step count!"

    def args(a=a, c0=c0, c1=c1, bkeys=(k[0], k[1]), belts=(3, 5), n1=2, gkeys=(k[2], k[3]), gelts=(7, 9), n2=2,
             weights=tuple(w), out=out, count=COUNT, scratch=s):
        return (a, c0, c1, ptrs(*bkeys), u32s(*belts), n1, ptrs(*gkeys), u32s(*gelts), n2,
                None if weights is None else ptrs(*weights), out, count, 1, scratch)

    cases = [
        ("no tables", args(), TABLES, e.bare),
        ("negative count", args(count=-1), BAD_COUNT),
        ("no baby steps", args(n1=0), steps),
        ("65 giant steps", args(n2=65), steps),
        ("null a", args(a=None), NULL),
        ("null weights", args(weights=None), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("an even baby element", args(belts=(3, 4)), ODD),
        ("an even giant element", args(gelts=(8, 9)), ODD),
        ("a null key at an element other than 1", args(bkeys=(k[0], None)),
         "A null key is accepted only where the element is 1!"),
        ("a baby step without a key and null c1", args(bkeys=(k[0], None), belts=(3, 1), c1=None), NULL),
        ("a baby step without a key, out is the scratch", args(bkeys=(k[0], None), belts=(3, 1), out=s), S_OUT),
        ("a giant step without a weight", args(weights=(w[0], w[1], None, None)),
         "A giant step has no present weight!"),
        ("out 8 words into a", args(out=a + e.OFF), OPERAND),
        ("c1 in the scratch", args(c1=s + 256), OPERAND),
        ("a giant key 8 words into out", args(gkeys=(k[2], out + e.OFF)), OPERAND),
        ("one null weight, another 8 words into out", args(weights=(None, w[1], w[2], out + e.OFF)), OPERAND),
        ("null c0, out is the scratch", args(c0=None, out=s), S_OUT),
        ("negative count and no baby steps", args(count=-1, n1=0), BAD_COUNT),
        ("no baby steps and null a", args(n1=0, a=None), steps),
        ("null a and a misaligned scratch", args(a=None, scratch=s + 8), NULL),
        ("a misaligned scratch and an even element", args(scratch=s + 8, belts=(4, 5)), ALIGN),
        ("an even element and a giant step without a weight", args(gelts=(7, 8), weights=(w[0], w[1], None, None)), ODD),
        ("an operand overlap and out is the scratch", args(a=s + 256, out=s), OPERAND),
    ]
    walk(e, "keyswitch_plan_linear_transform_bsgs", cases)
    walk(e, "keyswitch_plan_linear_transform_bsgs_rescale",
         [("no rescale_limbs", args(), RESCALE, e.plain), ("no tables", args(), TABLES, e.bare)] + cases[1:])


def relin_cases(e):
    x, y, key, out, s = (e.b(n) for n in ("x", "y", "key", "out", "scratch"))
    return [
        ("no tables", (x, y, key, out, COUNT, 1, s), TABLES, e.bare),
        ("negative count", (x, y, key, out, -1, 1, s), BAD_COUNT),
        ("null x", (None, y, key, out, COUNT, 1, s), NULL),
        ("null key", (x, y, None, out, COUNT, 1, s), NULL),
        ("null scratch", (x, y, key, out, COUNT, 1, None), NULL),
        ("misaligned scratch", (x, y, key, out, COUNT, 1, s + 8), ALIGN),
        ("x in the scratch", (s + 256, y, key, out, COUNT, 1, s), OPERAND),
        ("the key in the scratch", (x, y, s + 256, out, COUNT, 1, s), OPERAND),
        ("out exactly x", (x, y, key, x, COUNT, 1, s), None),
        ("out exactly y, which is x", (x, x, key, x, COUNT, 1, s), None),
        ("out 8 words into x", (x, y, key, x + e.OFF, COUNT, 1, s), OPERAND),
        ("out 8 words before y", (x, y + e.OFF, key, y, COUNT, 1, s), OPERAND),
        ("out exactly the key", (x, y, key, key, COUNT, 1, s), OPERAND),
        ("out is the scratch", (x, y, key, s, COUNT, 1, s), S_OUT),
        ("negative count and null x", (None, y, key, out, -1, 1, s), BAD_COUNT),
        ("null x and a misaligned scratch", (None, y, key, out, COUNT, 1, s + 8), NULL),
        ("a misaligned scratch with x inside", (s + 256, y, key, out, COUNT, 1, s + 8), ALIGN),
        ("x in the scratch and out is the scratch", (s + 256, y, key, s, COUNT, 1, s), OPERAND),
    ]


def test_multiply_relinearize(env):
    cases = relin_cases(env)
    walk(env, "keyswitch_plan_multiply_relinearize", cases)
    walk(env, "keyswitch_plan_multiply_relinearize_rescale",
         [("no rescale_limbs", cases[0][1], RESCALE, env.plain), ("no tables", cases[0][1], TABLES, env.bare)] + cases[1:])


def test_multiply_relinearize_sum(env):
    e = env
    x0, x1, y0, y1, key, out, s = (e.b(n) for n in ("x", "x1", "y", "y1", "key", "out", "scratch"))

    def args(xs=(x0, x1), ys=(y0, y1), terms=2, key=key, out=out, count=COUNT, scratch=s):
        return (None if xs is None else ptrs(*xs), None if ys is None else ptrs(*ys), terms, key, out, count, 1, scratch)

    cases = [
        ("no tables", args(), TABLES, e.bare),
        ("negative count", args(count=-1), BAD_COUNT),
        ("no terms", args(terms=0), "Invalid terms!"),
        ("33 terms", args(terms=33), "Invalid terms!"),
        ("null xs", args(xs=None), NULL),
        ("null key", args(key=None), NULL),
        ("a null term", args(ys=(y0, None)), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("the key in the scratch", args(key=s + 256), OPERAND),
        ("out exactly the key", args(out=key), OPERAND),
        ("a term in the scratch", args(xs=(x0, s + 256)), OPERAND),
        ("out exactly a term", args(out=y1), None),
        ("out exactly a term that appears twice", args(xs=(x0, x0), ys=(x0, y1), out=x0), None),
        ("out 8 words into a term", args(out=y1 + e.OFF), OPERAND),
        ("out is the scratch", args(out=s), S_OUT),
        ("negative count and no terms", args(count=-1, terms=0), BAD_COUNT),
        ("no terms and null key", args(terms=0, key=None), "Invalid terms!"),
        ("a null term and a misaligned scratch", args(xs=(x0, None), scratch=s + 8), NULL),
        ("null key and a misaligned scratch", args(key=None, scratch=s + 8), NULL),
        ("a misaligned scratch with a term inside", args(xs=(x0, s + 256), scratch=s + 8), ALIGN),
        ("a term in the scratch and out is the scratch", args(xs=(s + 256, x1), out=s), OPERAND),
    ]
    walk(e, "keyswitch_plan_multiply_relinearize_sum", cases)
    walk(e, "keyswitch_plan_multiply_relinearize_sum_rescale",
         [("no rescale_limbs", args(), RESCALE, e.plain), ("no tables", args(), TABLES, e.bare)] + cases[1:])


def test_relinearize(env):
    e = env
    c01, c2, key, out, s = (e.b(n) for n in ("c01", "c2", "key", "out", "scratch"))
    walk(e, "keyswitch_plan_relinearize", [
        ("no tables", (c01, c2, key, out, COUNT, 1, 1, s), TABLES, e.bare),
        ("negative count", (c01, c2, key, out, -1, 1, 1, s), BAD_COUNT),
        ("null c2", (c01, None, key, out, COUNT, 1, 1, s), NULL),
        ("misaligned scratch", (c01, c2, key, out, COUNT, 1, 1, s + 8), ALIGN),
        ("c2 in the scratch", (c01, s + 256, key, out, COUNT, 1, 1, s), OPERAND),
        ("out exactly c01, NTT form", (c01, c2, key, c01, COUNT, 1, 1, s), None),
        ("out exactly c01, coefficient form", (c01, c2, key, c01, COUNT, 0, 0, s), None),
        ("out 8 words into c01", (c01, c2, key, c01 + e.OFF, COUNT, 1, 1, s), OPERAND),
        ("out exactly c2", (c01, c2, key, c2, COUNT, 1, 1, s), OPERAND),
        ("c2 inside c01", (c01, c01 + e.OFF, key, out, COUNT, 1, 1, s), OPERAND),
        ("the key inside c2", (c01, c2, c2 + e.OFF, out, COUNT, 1, 1, s), OPERAND),
        ("out is the scratch", (c01, c2, key, s, COUNT, 1, 1, s), S_OUT),
        ("negative count and a misaligned scratch", (c01, c2, key, out, -1, 1, 1, s + 8), BAD_COUNT),
        ("a misaligned scratch with c2 inside", (c01, s + 256, key, out, COUNT, 1, 1, s + 8), ALIGN),
        ("c2 inside c01 and out is the scratch", (c01, c01 + e.OFF, key, s, COUNT, 1, 1, s), OPERAND),
    ])


def test_lift_small_and_lift_centred(env):
    e = env
    small, out = e.b("small"), e.b("out")
    lift = "The lift's input and output overlap!"
    walk(e, "keyswitch_plan_lift_small", [
        ("no tables", (small, out, 2, 1, 1), TABLES, e.bare),
        ("negative polys", (small, out, -1, 1, 1), "Invalid polys!"),
        ("null small", (None, out, 2, 1, 1), NULL),
        ("out 8 words into small", (small, small + 32, 2, 1, 1), lift),
        ("small inside out, q-base", (out + 32, out, 2, 0, 0), lift),
    ])
    t, bad = e.word(65537), e.word(1)
    walk(e, "keyswitch_plan_lift_centred", [
        ("no tables", (small, t, out, 2, 1, 1), TABLES, e.bare),
        ("t = 1", (small, bad, out, 2, 1, 1), "Invalid plaintext modulus!"),
        ("t from 2^(W-1) on", (small, e.word(1 << (e.bits - 1)), out, 2, 1, 1), "Invalid plaintext modulus!"),
        ("negative polys", (small, t, out, -1, 1, 1), "Invalid polys!"),
        ("null words", (None, t, out, 2, 1, 1), NULL),
        ("out 8 words into the words", (small, t, small + e.OFF, 2, 1, 1), lift),
        ("t = 1 and negative polys", (small, bad, out, -1, 1, 1), "Invalid plaintext modulus!"),
        ("negative polys and null out", (small, t, None, -1, 1, 1), "Invalid polys!"),
        ("no tables and t = 1", (small, bad, out, 2, 1, 1), TABLES, e.bare),
    ])


def test_multiply_plain(env):
    e = env
    ct, pt, out = e.b("ct"), e.b("pt"), e.b("out")
    walk(e, "keyswitch_plan_multiply_plain", [
        ("negative count", (ct, pt, out, -1, 1), BAD_COUNT),
        ("three plaintexts for two ciphertexts", (ct, pt, out, COUNT, 3), "Invalid plain_count!"),
        ("null pt", (ct, None, out, COUNT, 1), NULL),
        ("out exactly ct", (ct, pt, ct, COUNT, 1), None),
        ("out 8 words into ct", (ct, pt, ct + e.OFF, COUNT, 1), "out overlaps an operand!"),
        ("out exactly pt", (ct, pt, pt, COUNT, COUNT), "out overlaps an operand!"),
        ("negative count and null ct", (None, pt, out, -1, 1), BAD_COUNT),
        ("a wrong plain_count and null out", (ct, pt, None, COUNT, 3), "Invalid plain_count!"),
    ])


def test_generate_keys(env):
    e = env
    sk, s_from, errors, k0, k1, s = (e.b(n) for n in ("s", "s_from", "errors", "key0", "key1", "scratch"))
    level = "Keys are generated by the plan of the level they are laid out for!"

    def args(sk=sk, s_from=s_from, errors=errors, keys=(k0, k1), count=2, scratch=s):
        return (sk, s_from, errors, None if keys is None else ptrs(*keys), count, scratch)

    walk(e, "keyswitch_plan_generate_keys", [
        ("no tables", args(), TABLES, e.bare),
        ("negative keys", args(count=-1), "Invalid keys!"),
        ("a plan with wider keys", args(), level, e.wide_keys),
        ("null s", args(sk=None), NULL),
        ("null key list", args(keys=None), NULL),
        ("a null key", args(keys=(k0, None)), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("s in the scratch", args(sk=s + 256), S_OP),
        ("a key 8 words into the errors", args(keys=(k0, errors + 32)), "A key overlaps an operand!"),
        ("a key in the scratch", args(keys=(s + 256, k1)), "The scratch overlaps a key!"),
        ("two keys 8 words apart", args(keys=(k0, k0 + e.OFF)), "Two keys overlap!"),
        ("negative keys and null s", args(count=-1, sk=None), "Invalid keys!"),
        ("wider keys and null s", args(sk=None), level, e.wide_keys),
        ("a null key and a misaligned scratch", args(keys=(None, k1), scratch=s + 8), NULL),
        ("a misaligned scratch with s inside", args(sk=s + 256, scratch=s + 8), ALIGN),
        ("a key over s and s_from in the scratch", args(keys=(sk + e.OFF, k1), s_from=s + 256), "A key overlaps an operand!"),
        ("a key in the scratch and two keys 8 words apart", args(keys=(s + 256, s + 256 + e.OFF)),
         "The scratch overlaps a key!"),
    ])


def encrypt_cases(e, first):
    errors, msg, out, s = (e.b(n) for n in ("errors", "message", "out", "scratch"))
    return [
        ("no tables", (first, errors, msg, out, COUNT, s), TABLES, e.bare),
        ("negative count", (first, errors, msg, out, -1, s), BAD_COUNT),
        ("null first operand", (None, errors, msg, out, COUNT, s), NULL),
        ("null out", (first, errors, msg, None, COUNT, s), NULL),
        ("misaligned scratch", (first, errors, msg, out, COUNT, s + 8), ALIGN),
        ("the errors in the scratch", (first, s + 256, msg, out, COUNT, s), OPERAND),
        ("the message 8 words into out", (first, errors, out + e.OFF, out, COUNT, s), OPERAND),
        ("out exactly the first operand", (first, errors, msg, first, COUNT, s), OPERAND),
        ("null message, out is the scratch", (first, errors, None, s, COUNT, s), S_OUT),
        ("negative count and null out", (first, errors, msg, None, -1, s), BAD_COUNT),
        ("null out and a misaligned scratch", (first, errors, msg, None, COUNT, s + 8), NULL),
        ("a misaligned scratch with the errors inside", (first, s + 256, msg, out, COUNT, s + 8), ALIGN),
        ("the message in out and out is the scratch", (first, errors, s + e.OFF, s, COUNT, s), OPERAND),
    ]


def test_encrypt_symmetric(env):
    walk(env, "keyswitch_plan_encrypt_symmetric", encrypt_cases(env, env.b("s")))


def test_encrypt_public(env):
    walk(env, "keyswitch_plan_encrypt_public", encrypt_cases(env, env.b("pk")))


def test_phase(env):
    e = env
    ct, sk, out, s = (e.b(n) for n in ("ct", "s", "out", "scratch"))
    walk(e, "keyswitch_plan_phase", [
        ("no tables, coefficient input", (ct, sk, out, COUNT, 2, 0, 1, s), TABLES, e.bare),
        ("four components", (ct, sk, out, COUNT, 4, 1, 1, None), "Invalid components!"),
        ("negative count", (ct, sk, out, -1, 2, 1, 1, None), BAD_COUNT),
        ("null ct", (None, sk, out, COUNT, 2, 1, 1, None), NULL),
        ("null scratch, coefficient input", (ct, sk, out, COUNT, 2, 0, 1, None), NULL),
        ("misaligned scratch, coefficient input", (ct, sk, out, COUNT, 2, 0, 1, s + 8), ALIGN),
        ("out exactly ct, NTT input", (ct, sk, ct, COUNT, 3, 1, 1, None), None),
        ("out exactly ct, coefficient input", (ct, sk, ct, COUNT, 2, 0, 1, s), "out overlaps an operand!"),
        ("out 8 words into ct", (ct, sk, ct + e.OFF, COUNT, 2, 1, 1, None), "out overlaps an operand!"),
        ("out exactly s", (ct, sk, sk, COUNT, 2, 1, 1, None), "out overlaps an operand!"),
        ("s in the scratch", (ct, s + 256, out, COUNT, 2, 0, 1, s), OPERAND),
        ("out is the scratch", (ct, sk, s, COUNT, 2, 0, 1, s), S_OUT),
        ("a misaligned scratch ignored for NTT input, out exactly s", (ct, sk, sk, COUNT, 2, 1, 1, s + 8),
         "out overlaps an operand!"),
        ("four components and negative count", (ct, sk, out, -1, 4, 1, 1, None), "Invalid components!"),
        ("negative count and null ct", (None, sk, out, -1, 2, 1, 1, None), BAD_COUNT),
        ("null ct and a misaligned scratch", (None, sk, out, COUNT, 2, 0, 1, s + 8), NULL),
        ("a misaligned scratch and out exactly s", (ct, sk, sk, COUNT, 2, 0, 1, s + 8), ALIGN),
        ("out exactly s and s in the scratch", (ct, s + 256, s + 256, COUNT, 2, 0, 1, s), "out overlaps an operand!"),
    ])


def test_bfv_decrypt(env):
    e = env
    ct, sk, msg, noise, s, ks = (e.b(n) for n in ("ct", "s", "message", "noise", "scratch", "ks_scratch"))
    decode = "decode input and output overlap!"

    def args(ct=ct, plan=None, sk=sk, msg=msg, noise=noise, count=COUNT, components=2, input_ntt=0, scratch=s, ks=ks):
        return (ct, (plan or e.plan)._h, sk, msg, noise, count, components, input_ntt, scratch, ks)

    cases = [
        ("a plan of another q-base", args(plan=e.other), MATCH),
        ("a plan without tables", args(plan=e.bare), MATCH),
        ("negative count", args(count=-1), BAD_COUNT),
        ("null scratch", args(scratch=None), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("null message", args(msg=None), NULL),
        ("the message in the scratch", args(msg=s + e.OFF), decode),
        ("noise_max in the message", args(noise=msg + e.OFF), decode),
        ("four components", args(components=4), "Invalid components!"),
        ("the message 8 words into ct", args(msg=ct + e.OFF), OPERAND),
        ("noise_max in s", args(noise=sk + e.OFF), OPERAND),
        ("the message in the phase's scratch", args(msg=ks + 256), OPERAND),
        ("null noise_max, null ct", args(noise=None, ct=None), NULL),
        ("null phase scratch, coefficient input", args(ks=None), NULL),
        ("misaligned phase scratch", args(ks=ks + 8), ALIGN),
        ("ct in the scratch", args(ct=s + e.OFF), "out overlaps an operand!"),
        ("another plan and negative count", args(plan=e.other, count=-1), MATCH),
        ("negative count and null scratch", args(count=-1, scratch=None), BAD_COUNT),
        ("a misaligned scratch and null message", args(scratch=s + 8, msg=None), ALIGN),
        ("the message in the scratch and in ct", args(msg=s + e.OFF, ct=s + 2 * e.OFF), decode),
        ("four components and the message in ct", args(components=4, msg=ct + e.OFF), "Invalid components!"),
    ]
    walk(e, "bfv_plan_decrypt", [(w, a, m, e.bfv) for w, a, m in cases])


def test_bfv_multiply_relinearize(env):
    e = env
    x, y, key, out, s, ks = (e.b(n) for n in ("x", "y", "key", "out", "scratch", "ks_scratch"))

    def args(x=x, y=y, plan=None, key=key, out=out, count=COUNT, scratch=s, ks=ks):
        return (x, y, (plan or e.plan)._h, key, out, count, 1, 1, scratch, ks)

    cases = [
        ("a plan of another q-base", args(plan=e.other), MATCH),
        ("null key", args(key=None), NULL),
        ("negative count", args(count=-1), BAD_COUNT),
        ("misaligned key-switching scratch", args(ks=ks + 8), ALIGN),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("x in the scratch", args(x=s + 256), OPERAND),
        ("out exactly x", args(out=x), None),
        ("out 8 words into x", args(out=x + e.OFF), OPERAND),
        ("out is the scratch", args(out=s), S_OUT),
        ("y in the key-switching scratch", args(y=ks + 256), OPERAND),
        ("the key in the scratch", args(key=s + 256), OPERAND),
        ("the key 8 words into x", args(key=x + e.OFF), OPERAND),
        ("out is the key-switching scratch", args(out=ks), S_OUT),
        ("the two scratches overlap", args(ks=s + 256), S_OUT),
        ("another plan and negative count", args(plan=e.other, count=-1), MATCH),
        ("negative count and a misaligned key-switching scratch", args(count=-1, ks=ks + 8), BAD_COUNT),
        ("a misaligned key-switching scratch and out in x", args(ks=ks + 8, out=x + e.OFF), ALIGN),
        ("out is the scratch and the key in the key-switching scratch", args(out=s, key=ks + 256), S_OUT),
    ]
    walk(e, "bfv_plan_multiply_relinearize", [(w, a, m, e.bfv) for w, a, m in cases])


def test_bfv_multiply_relinearize_sum(env):
    e = env
    x0, x1, y0, y1, key, out, s, ks = (e.b(n) for n in ("x", "x1", "y", "y1", "key", "out", "scratch", "ks_scratch"))

    def args(xs=(x0, x1), ys=(y0, y1), terms=2, plan=None, key=key, out=out, count=COUNT, scratch=s, ks=ks):
        return (None if xs is None else ptrs(*xs), ptrs(*ys), terms, (plan or e.plan)._h, key, out, count, 1, 1, scratch, ks)

    cases = [
        ("a plan of another q-base", args(plan=e.other), MATCH),
        ("null key", args(key=None), NULL),
        ("negative count", args(count=-1), BAD_COUNT),
        ("misaligned key-switching scratch", args(ks=ks + 8), ALIGN),
        ("no terms", args(terms=0), "Invalid terms!"),
        ("null xs", args(xs=None), NULL),
        ("a null term", args(ys=(y0, None)), NULL),
        ("misaligned scratch", args(scratch=s + 8), ALIGN),
        ("a term in the scratch", args(xs=(x0, s + 256)), OPERAND),
        ("out exactly a term", args(out=y1), None),
        ("out 8 words into a term", args(out=y1 + e.OFF), OPERAND),
        ("out is the scratch", args(out=s), S_OUT),
        ("a term in the key-switching scratch", args(ys=(ks + 256, y1)), OPERAND),
        ("the key 8 words into out", args(key=out + e.OFF), OPERAND),
        ("out is the key-switching scratch", args(out=ks), S_OUT),
        ("null key and no terms", args(key=None, terms=0), NULL),
        ("a misaligned key-switching scratch and no terms", args(ks=ks + 8, terms=0), ALIGN),
        ("a null term and a misaligned scratch", args(xs=(x0, None), scratch=s + 8), NULL),
        ("out is the scratch and the key in the key-switching scratch", args(out=s, key=ks + 256), S_OUT),
    ]
    walk(e, "bfv_plan_multiply_relinearize_sum", [(w, a, m, e.bfv) for w, a, m in cases])


def test_bfv_encoder(env):
    e = env
    values, plain, s = e.b("values"), e.b("plain"), e.b("scratch")
    enc = e.encoder.plan
    walk(e, "bfv_encoder_encode", [(w, a, m, enc) for w, a, m in [
        ("negative count", (values, plain, -1), BAD_COUNT),
        ("null values", (None, plain, COUNT), NULL),
        ("plain 8 words into the values", (values, values + e.OFF, COUNT), "encode input and output overlap!"),
        ("negative count and null plain", (values, None, -1), BAD_COUNT),
    ]])
    decode = "decode input and output overlap!"
    walk(e, "bfv_encoder_decode", [(w, a, m, enc) for w, a, m in [
        ("negative count", (plain, values, -1, s), BAD_COUNT),
        ("null scratch", (plain, values, COUNT, None), NULL),
        ("misaligned scratch", (plain, values, COUNT, s + 8), ALIGN),
        ("the values 8 words into plain", (plain, plain + e.OFF, COUNT, s), decode),
        ("plain is the scratch", (s, values, COUNT, s), S_OP),
        ("the values in the scratch", (plain, s + e.OFF, COUNT, s), S_OP),
        ("negative count and null plain", (None, values, -1, s), BAD_COUNT),
        ("null values and a misaligned scratch", (plain, None, COUNT, s + 8), NULL),
        ("a misaligned scratch with plain inside", (s + 256, values, COUNT, s + 8), ALIGN),
        ("the values in plain, both in the scratch", (s, s + e.OFF, COUNT, s), decode),
    ]])
