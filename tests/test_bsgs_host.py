"""KeySwitchPlan.linear_transform_bsgs without a GPU: (a) its arithmetic in Python integers (tests/bsgs_exact.py) -- the
words of the fused giant-step sum against the definition's per-step sums, and the ring identity behind adding v_g[0] with
multiplier 1; (b) the text of the three new kernels compiled for the host and run under AddressSanitizer and UBSan
(tests/cpp/emulate_bsgs.cpp through tests/bsgs_emulator.py); the scratch size, which is host arithmetic."""
import random

import pytest

from bsgs_emulator import run_emulator
from bsgs_exact import giant_definition, giant_step_identity, giant_words

# primes = 1 mod 32: every ring up to N = 16 has its roots, though the identities below need none
TINY_Q, TINY_P = [97, 193, 257, 353], [449, 577]


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("top", [False, True])
def test_the_fused_giant_sum_is_the_sum_of_the_giant_steps(W, top):
    """any words in, 64 giant steps and 64 digits at the most: the unreduced terms stay below 3 q, the carry word of the
    across-g accumulator at 64 at most (asserted inside giant_words), and the one fold returns the definition's word"""
    rng = random.Random(W + top)
    mask = (1 << W) - 1
    for trial in range(40):
        q = ((1 << (W - 2)) - 1 - 2 * rng.randrange(1 << (W - 6 if top else 8))) | 1
        if not top:
            q >>= 1
            q |= 1
        n2k, plain, D = rng.choice([(1, 0, 1), (2, 1, 3), (64, 0, 2), (40, 24, 1), (0, 5, 2), (3, 2, 64)])

        def word():
            return rng.choice([0, mask, q - 1, q, rng.randrange(1 << W)])
        if trial % 8 == 0:
            def word():  # noqa: F811 -- the largest sums
                return mask
        digits = [[word() for _ in range(D)] for _ in range(n2k)]
        keys = [[word() for _ in range(D)] for _ in range(n2k)]
        v0, pl = [word() for _ in range(n2k)], [word() for _ in range(plain)]
        assert giant_words(digits, keys, v0, pl, q, W) == giant_definition(digits, keys, v0, pl, q)


@pytest.mark.parametrize("n_power", [2, 3, 4])
@pytest.mark.parametrize("alpha", [1, 2])
def test_the_first_component_joins_with_multiplier_one(n_power, alpha):
    """s_g[0] + s_g[1] s = sigma_g(V0 + V1 s) - sigma_g(conv s) modulo P Q, exactly: V0 is at scale P already, and what the
    re-decomposition loses is the centred residue of V1 modulo P alone"""
    n = 1 << n_power
    rng = random.Random(n_power * 10 + alpha)
    P = TINY_P[0] * TINY_P[1]
    for k in (5, 2 * n - 1, pow(5, 3, 2 * n), 1):
        left, right, conv = giant_step_identity(rng, n, TINY_Q, TINY_P, alpha, k)
        assert left == right
        assert all(2 * abs(c) <= P for c in conv) and any(c != 0 for c in conv)
    # with P as the multiplier on V0 (what the c0 term of a baby step takes) the identity fails: the check is not vacuous
    left, right, _ = giant_step_identity(rng, n, TINY_Q, TINY_P, alpha, 5, multiplier=P)
    assert left != right


@pytest.mark.parametrize("which", ["scale", "sum", "giant"])
def test_the_kernels_on_the_host_under_sanitizers(tmp_path, which):
    out = run_emulator(tmp_path, which)
    assert "WRONG" not in out and "W=64" in out and "W=32" in out


def test_the_scratch_size_and_its_limits(pkg):
    """bsgs_scratch_bytes is host arithmetic: u (2 n1) + v (2 n2) components of count M N words, t (n2 count L N) and the
    digits (D n2 count M N), each rounded up to 256 bytes"""
    g = pkg
    g.load_library()
    L, K, alpha, n_power, count, n1, n2 = 6, 2, 2, 9, 3, 5, 4
    M, D, n = L + K, 3, 1 << n_power
    for bits in (64, 32):
        plan = g.KeySwitchPlan.__new__(g.KeySwitchPlan)
        plan._h = None  # nothing to destroy
        plan.q_count, plan.p_count, plan.alpha, plan.n_power, plan.bits = L, K, alpha, n_power, bits
        word = bits // 8
        want = sum((w * word + 255) // 256 * 256 for w in (2 * n1 * count * M * n, 2 * n2 * count * M * n,
                                                           n2 * count * L * n, D * n2 * count * M * n))
        assert plan.bsgs_scratch_bytes(count, n1, n2) == want
        assert plan.bsgs_scratch_bytes(0, 64, 4) == 0
        for bad in ((257, 1), (65, 1), (1, 65), (64, 5), (1, 0), (0, 1)):
            with pytest.raises(ValueError):
                plan.bsgs_scratch_bytes(count, *bad)
        with pytest.raises(ValueError):
            plan.bsgs_scratch_bytes(-1, 1, 1)
        plan._h = None  # nothing to destroy
