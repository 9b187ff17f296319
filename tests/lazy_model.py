"""Exact-integer statement of the contracts of gpu-ntt_amd/csrc/lazy.hpp, and the operands that carry a lazy value to the
edges of its range (tests/test_gpu_lazy_arith.py runs them through tests/cpp/lazy_arith_probe.hip on the device,
tests/test_lazy_model_host.py checks on the CPU that they do reach the edges).

Every function here works on Python integers -- plain ones, or numpy arrays of dtype=object, which hold plain integers and
apply the same operators element by element (no fixed-width arithmetic anywhere).  What is stated is each primitive's
CONTRACT as the header words it ("result in [0, 4q) for any x < 2^64"), not its instruction sequence; the two places
where the header documents a formula (the dropped-partial-product quotient of the 64-bit product, the quotient estimate
of the one-multiply normalisation) are restated for the host test, which uses them to show that the generated operands
are the hard ones and that the constants the header computes are the documented ones.
"""
import random
import struct
from collections import namedtuple

import numpy as np

MAGIC = 0x424F52505A414C4C
WAVE = 64             # cases per block: one wave, one modulus (uniform families), one wave-uniform twiddle
LANES_PER_MODULUS = 256
MAX_CASES = 1 << 18

Family = namedtuple("Family", "name id W lim vq tb max_bit ks norms")
# the Mod<...> specialisations of lazy.hpp: (word, LIMIT, per-lane moduli) -> product bound TB, widest `bit`,
# the K of csub<K> / csub_c<K> and the B of normalize<B> the probe instantiates for it
FAMILIES = {f.name: f for f in (
    Family("m64_16", 0, 64, 16, False, 4, 60, (1, 2, 4, 8, 16), (2, 4, 8, 16)),
    Family("m64_31", 1, 64, 31, False, 4, 60, (1, 2, 4, 8, 16), (2, 4, 8, 16, 31, 32)),
    Family("m64_8", 2, 64, 8, False, 4, 61, (1, 2, 4, 8), (2, 4, 8)),
    Family("m64_4", 3, 64, 4, False, 2, 62, (1, 2, 4), (2, 4)),
    Family("m64_4v", 4, 64, 4, True, 2, 62, (1, 2, 4), (2, 4)),
    Family("m64_16v", 5, 64, 16, True, 4, 60, (1, 2, 4, 8, 16), (2, 4, 8, 16)),
    Family("m64_8v", 6, 64, 8, True, 4, 61, (1, 2, 4, 8), (2, 4, 8)),
    Family("m32_4", 7, 32, 4, False, 2, 30, (1, 2, 4), (2, 4)),
    Family("m32_4v", 8, 32, 4, True, 2, 30, (1, 2, 4), (2, 4)),
    Family("m32_8", 9, 32, 8, False, 2, 29, (1, 2, 4, 8), (2, 4, 8)),
)}

# (family, q, x, w, acc) that once failed on the device: kept in every later case set.  None so far.
FIXED_CASES = []


# ------------------------------------------------------------------------------------------------- contracts
def product_ok(res, acc, x, w, q, tb, W):
    """mul / mul_acc / mul_acc_raw: (res - acc) mod 2^W = (x w mod q) + e q with 0 <= e < tb, for ANY word x"""
    d = (res - acc) % (1 << W) - (x * w) % q
    return (d % q == 0) & (d // q >= 0) & (d // q < tb)


def mulc_ok(res, x, w, q, tb, W):
    """mulc: the bitwise complement of such a product"""
    return product_ok((1 << W) - 1 - res, 0, x, w, q, tb, W)


def shl1_add(x, k, W):
    return (2 * x + k) % (1 << W)


def xad_not(w, u):
    return (u - w - 1) % (1 << 32)


def csub(x, k, q):
    """csub<K>: x - K q if x >= K q, else x.  (32-bit words, min form: stated for x < 2 K q -- csub_domain)"""
    return np.where(x >= k * q, x - k * q, x) if isinstance(x, np.ndarray) else (x - k * q if x >= k * q else x)


def csub_domain(x, k, q, W):
    return (x < 2 * k * q) if W == 32 else (x == x)


def csub_c_of_complement(x, k, q):
    """csub_c<K>: csub<K> on complemented values (32-bit words) -- handed ~x, it returns ~csub<K>(x); same domain"""
    return 0xFFFFFFFF - csub(x, k, q)


def reduce_2q_ok(res, x, q):
    """reduce_2q: congruent to x, in [0, 2q)"""
    return ((res - x) % q == 0) & (res >= 0) & (res < 2 * q)


def reduce_2q_domain(x, q, W):
    """64-bit words: x < 32 q (and a word); 32-bit words: any word"""
    return (x < 32 * q) if W == 64 else (x == x)


def normalize(x, q):
    """normalize<B>: the canonical residue, for every x < B q"""
    return x % q


# ------------------------------------------------------------------- the two formulas the header documents
def documented_quotient(x, wp):
    """qh = x1 wp1 + hi32(x1 wp0) + hi32(x0 wp1) (lazy.hpp, mul_acc_raw): hi64(x wp) without its low partial products"""
    x0, x1, p0, p1 = x & 0xFFFFFFFF, x >> 32, wp & 0xFFFFFFFF, wp >> 32
    return x1 * p1 + ((x1 * p0) >> 32) + ((x0 * p1) >> 32)


def documented_product(x, w, wp, q):
    """T = x w - qh q, and how far qh falls short of hi64(x wp)"""
    qh = documented_quotient(x, wp)
    return x * w - qh * q, ((x * wp) >> 64) - qh


NormConst = namedtuple("NormConst", "sh c M hi")


def make_norm_const(q, bit, W=64):
    """lazy.hpp: make_norm_const (64-bit words) / norm_const_of (32-bit words: M = floor(2^32 / q), no shifts)"""
    if W == 32:
        return NormConst(0, 0, (1 << 32) // q if q >= 3 else 0, 0)
    if q < 3 or bit < 2 or bit > 61:
        return NormConst(0, 0, 0, 0)
    hi = 1 if bit >= 48 else 0
    sh = 32 if hi else max(bit - 27, 0)
    qt = (q >> sh) + (1 if sh > 0 else 0)
    c = bit - 1 - sh
    return NormConst(sh, c, min((1 << (32 + c)) // qt, 0xFFFFFFFF), hi)


def documented_reduce_2q(x, q, nc):
    """k = ((x >> sh) M) >> (32 + c), x - k q"""
    return x - ((((x >> nc.sh) & 0xFFFFFFFF) * nc.M) >> (32 + nc.c)) * q


def shoup(w, q, W):
    return (w << W) // q


# ------------------------------------------------------------------------------------------------- moduli
def modulus_candidates(fam, find_ntt_prime, rng):
    """odd values of every true width 2 .. MAX_BIT: the largest (2^b - 1, and from 41 bits the largest clear of the double
    rounding behind Modulus<T>::bit), the smallest, an NTT prime, seeded random ones and, from 50 bits, 2^b - 107, whose
    `bit` is over-stated by one (and the top of the 31 q < 2^64 range for that family)"""
    qmax = ((1 << 64) - 1) // 31 if fam.lim == 31 else (1 << fam.max_bit) - 1
    out = []
    for b in range(2, fam.max_bit + 1):
        lo, hi = (1 << (b - 1)) + 1, min((1 << b) - 1, qmax)
        if lo > hi:
            continue
        hi_odd = hi if hi & 1 else hi - 1
        c = [hi_odd, lo]
        if b > 40:
            c.append(min((1 << b) - (1 << (b - 40)) - 1, hi_odd))
        p = find_ntt_prime(b)
        if p is not None and p <= hi:
            c.append(p)
        c += [rng.randrange(lo, hi + 1) | 1 for _ in range(2)]
        if b >= 50:
            c.append((1 << b) - 107)
        for q in c:
            if lo <= q <= hi and q not in out:
                out.append(q)
    return out


def family_moduli(fam, bit_of, find_ntt_prime, seed=0x1A27):
    """[(q, bit)] of a family, by STATED width: bit_of(q, W) is the library's own Modulus<T>::bit, or None where the
    library refuses the modulus.  A modulus goes to the family its stated width selects, or nowhere."""
    rng = random.Random(seed + fam.id)
    out = []
    for q in modulus_candidates(fam, find_ntt_prime, rng):
        bit = bit_of(q, fam.W)
        if bit is None or bit > fam.max_bit:
            continue
        out.append((q, bit))
    return out


# ------------------------------------------------------------------------------------------------- operands
def edge_words(q, W, rng):
    """x = k q + d for k = 0 .. 32 and d = -2 .. 2 (clipped to the word), the top of the word, words within 2^40 of it,
    words with a half of all ones or all zeros; then seeded random words"""
    top = (1 << W) - 1
    half = W // 2
    hm = (1 << half) - 1
    xs = []
    for k in range(33):
        for d in (-2, -1, 0, 1, 2):
            xs.append(min(max(k * q + d, 0), top))
    xs += [top, top - 1, top - rng.getrandbits(min(40, W - 1)), top - rng.getrandbits(min(40, W - 1)), top - rng.getrandbits(20),
           top - rng.getrandbits(8), 1 << (W - 1), (1 << (W - 1)) - 1]
    a, b = rng.getrandbits(half), rng.getrandbits(half)
    xs += [hm << half, hm, a << half, (a << half) | hm, (hm << half) | b, b]
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def special_twiddles(q):
    return [min(max(w, 1), q - 1) for w in (1, 2, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1)]


def hard_products(q, W, rng, w=None, tries=300):
    """(x, w) near the top of the word whose documented quotient is 2 short, and one whose product reaches 3 q (64-bit
    words).  Whether a product can reach 3 q depends on the twiddle far more than on x (for most twiddles none does, for
    the others a few per cent of the words near the top do): without a given w, twiddles are drawn until one does.
    None where the search does not find one."""
    short2 = t3q = None
    for _ in range(1 if w is not None else 40):
        ww = w if w is not None else rng.randrange(1, q)
        for _ in range(tries if w is not None else 60):
            x = (1 << W) - 1 - rng.getrandbits(rng.choice((8, 20, 33, 40)))
            t, short = documented_product(x, ww, shoup(ww, q, W), q)
            if short == 2 and short2 is None:
                short2 = (x, ww)
            if t >= 3 * q and t3q is None:
                t3q = (x, ww)
            if short2 is not None and t3q is not None:
                return short2, t3q
    return short2, t3q


Cases = namedtuple("Cases", "fam ncase nuni x acc q bit w wp qb bitb wu wpu")


def generate(fam, moduli, seed=0xC0FFEE):
    """The case set of one family: LANES_PER_MODULUS cases per modulus in blocks of WAVE.  Every block has one wave-uniform
    twiddle (the special ones rotate over the blocks of a stated width, then random ones; 64-bit words: the last block of
    a modulus takes a twiddle whose products reach 3 q) and ends with two lanes for the hard x of that twiddle.
    Accumulators rotate over 0, (LIMIT - TB) q - 1 and random words.  VQ families: the same cases again behind them, shuffled, so that the lanes of a wave hold different moduli (no UNI products there: nuni)."""
    rng = random.Random(seed + fam.id)
    W, top = fam.W, (1 << fam.W) - 1
    nblk = LANES_PER_MODULUS // WAVE
    hard = 2 if W == 64 else 0  # lanes per block kept for the block twiddle's hard products
    per = WAVE - hard
    x, acc, q_, bit_, w_, wp_, qb, bitb, wu, wpu = ([] for _ in range(10))
    rot = {}
    for q, bit in moduli:
        tws = special_twiddles(q)

        def twiddle(i):
            return tws[i % 8] if i % 8 < len(tws) else rng.randrange(1, q)

        lanes = [(fx, fw, fa) for (ff, fq, fx, fw, fa) in FIXED_CASES if ff == fam.name and fq == q]
        hard_w = None
        if W == 64:
            found = hard_products(q, W, rng)
            lanes += [(hx, hw, None) for (hx, hw) in filter(None, found)]
            hard_w = found[1][1] if found[1] is not None else None
        xs = edge_words(q, W, rng)
        assert len(lanes) + len(xs) <= nblk * per, "no room for every edge word (too many FIXED_CASES for this modulus)"
        lanes += [(ex, twiddle(i), None) for i, ex in enumerate(xs)]  # EVERY edge word, then random words
        while len(lanes) < nblk * per:
            lanes.append((rng.getrandbits(W), twiddle(len(lanes)), None))
        default_acc = (0, (fam.lim - fam.tb) * q - 1, None, None)
        for b in range(nblk):
            r = rot.get(bit, 0)
            rot[bit] = r + 1
            u = hard_w if (hard_w is not None and b == nblk - 1) else twiddle(r)
            blk = lanes[b * per:(b + 1) * per]
            if hard:
                for hit in hard_products(q, W, rng, w=u, tries=300):
                    blk.append((hit[0] if hit is not None else top - rng.getrandbits(33), rng.randrange(1, q), None))
            assert len(blk) == WAVE
            for i, (cx, cw, ca) in enumerate(blk):
                if ca is None:
                    ca = default_acc[(i + b) % 4]
                x.append(cx)
                acc.append(rng.getrandbits(W) if ca is None else ca % (1 << W))
                q_.append(q)
                bit_.append(bit)
                w_.append(cw)
                wp_.append(shoup(cw, q, W))
            qb.append(q)
            bitb.append(bit)
            wu.append(u)
            wpu.append(shoup(u, q, W))
    nuni = len(x)
    if fam.vq:
        perm = list(range(nuni))
        rng.shuffle(perm)
        for arr in (x, acc, q_, bit_, w_, wp_):
            arr += [arr[j] for j in perm]
        for arr in (qb, bitb, wu, wpu):  # the block words of the mixed part: read by nothing that is compared
            arr += arr[:]
    assert len(x) % WAVE == 0 and len(x) <= MAX_CASES, len(x)
    return Cases(fam, len(x), nuni, x, acc, q_, bit_, w_, wp_, qb, bitb, wu, wpu)


def write_cases(c, path):
    t = np.uint64 if c.fam.W == 64 else np.uint32
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", MAGIC, c.fam.id, c.ncase, c.nuni, 0, 0, 0, 0))
        for arr in (c.x, c.acc, c.q, c.bit, c.w, c.wp, c.qb, c.bitb, c.wu, c.wpu):
            f.write(np.array(arr, dtype=t).tobytes())


def read_results(path, fam, ncase):
    """{record name: object array of ncase Python integers}"""
    t = np.dtype("<u8" if fam.W == 64 else "<u4")
    with open(path, "rb") as f:
        magic, fid, n, nrec = struct.unpack("<4Q", f.read(32))
        assert (magic, fid, n) == (MAGIC, fam.id, ncase), (magic, fid, n)
        out = {}
        for _ in range(nrec):
            name = f.read(16).rstrip(b"\0").decode()
            buf = f.read(t.itemsize * n)
            assert len(buf) == t.itemsize * n, "result file cut short in " + name
            out[name] = np.array(np.frombuffer(buf, dtype=t).tolist(), dtype=object)
        assert f.read(1) == b"", "bytes behind the last record"
    return out


def expected_records(fam):
    """the record names the probe writes for a family"""
    r = ["mul_u", "mul_v", "macc_u", "macc_v", "maccz_u", "maccz_v"]
    if fam.W == 64:
        if fam.lim == 4:
            r += ["raw_u", "raw_v"]
        r += ["csub%d" % k for k in fam.ks] + ["shl1", "red2q", "red2q_hi"]
        for b in fam.norms:
            r += ["norm%d" % b] + (["norm%d_hi" % b] if b > 4 else [])
    else:
        r += ["mulc_u", "mulc_v"] + ["csub%d" % k for k in fam.ks] + ["csubc%d" % k for k in fam.ks]
        r += ["shl1", "red2q"] + ["norm%d" % b for b in fam.norms] + ["xad_not"]
    return r


# ------------------------------------------------------------------------- every result word against its contract
def verify(c, res):
    """Compare EVERY word the probe wrote for the case set `c` with its contract; returns the list of failures (strings
    naming the record, how many words fail and the first failing case), empty when the device meets every contract."""
    fam, W, n, nu = c.fam, c.fam.W, c.ncase, c.nuni
    top = (1 << W) - 1

    def obj(a):
        return np.array(a, dtype=object)

    x, acc, q, bit, w = obj(c.x), obj(c.acc), obj(c.q), obj(c.bit), obj(c.w)
    wu = obj([c.wu[i // WAVE] for i in range(nu)])
    ku = obj([c.wpu[i // WAVE] for i in range(n)])
    everywhere = np.ones(n, dtype=bool)
    fails = []
    if sorted(res) != sorted(expected_records(fam)):
        return ["records %s, expected %s" % (sorted(res), sorted(expected_records(fam)))]

    def check(name, ok, dom=everywhere, m=n):
        ok, dom = np.asarray(ok, dtype=bool), np.asarray(dom, dtype=bool)[:m]
        if not dom.any():
            fails.append("%s: no case inside its domain" % name)
        bad = np.flatnonzero(dom & ~ok)
        if bad.size:
            i = int(bad[0])
            wi = wu[i] if name.endswith("_u") else w[i]
            fails.append("%s/%s: %d of %d words break the contract; first: case %d q=%d bit=%d x=%d w=%d acc=%d got=%d"
                         % (fam.name, name, bad.size, int(dom.sum()), i, q[i], bit[i], x[i], wi, acc[i], res[name][i]))

    for name, a, tb in (("mul", 0, fam.tb), ("macc", acc, fam.tb), ("maccz", 0, fam.tb), ("raw", acc, 4)):
        if name + "_u" not in res:
            continue
        au = a if isinstance(a, int) else a[:nu]
        check(name + "_u", product_ok(res[name + "_u"][:nu], au, x[:nu], wu, q[:nu], tb, W), m=nu)
        check(name + "_v", product_ok(res[name + "_v"], a, x, w, q, tb, W))
        if nu < n and res[name + "_u"][nu:].any():
            fails.append("%s_u: words written behind the %d cases it covers" % (name, nu))
    if W == 32:
        check("mulc_u", mulc_ok(res["mulc_u"][:nu], x[:nu], wu, q[:nu], fam.tb, W), m=nu)
        check("mulc_v", mulc_ok(res["mulc_v"], x, w, q, fam.tb, W))
        check("xad_not", res["xad_not"] == xad_not(x, acc))
    for k in fam.ks:
        assert k * max(c.q) <= top  # kq(K) itself is a word
        check("csub%d" % k, res["csub%d" % k] == csub(x, k, q), csub_domain(x, k, q, W))
        if W == 32:
            # the probe hands csub_c the complement of x, so its edges are the same k q - 1 / k q words
            check("csubc%d" % k, res["csubc%d" % k] == csub_c_of_complement(x, k, q), csub_domain(x, k, q, W))
    check("shl1", res["shl1"] == shl1_add(x, acc if fam.vq else ku, W))
    has_nc = (bit <= 61) if W == 64 else everywhere  # make_norm_const: no record above 61 bits (LIMIT 4 never asks)
    hi = (bit >= 48) & (bit <= 61)  # nc.hi: the probe runs the HI forms on those moduli only and leaves 0 elsewhere
    check("red2q", reduce_2q_ok(res["red2q"], x, q), reduce_2q_domain(x, q, W) & has_nc)
    if W == 64:
        check("red2q_hi", reduce_2q_ok(res["red2q_hi"], x, q), reduce_2q_domain(x, q, W) & has_nc & hi)
    for b in fam.norms:
        check("norm%d" % b, res["norm%d" % b] == normalize(x, q), x < b * q)
        if W == 64 and b > 4:
            check("norm%d_hi" % b, res["norm%d_hi" % b] == normalize(x, q), (x < b * q) & hi)
    for name in res:
        if name.endswith("_hi") and res[name][~np.asarray(hi, dtype=bool)].any():
            fails.append("%s: words written for moduli without nc.hi" % name)
    return fails
