"""Integer model of the lazy sums of lodestar_amd/csrc/lsg_fp_pair.hpp: the grouped carry at its
limit (three values added, three subtracted) and the small-multiple-with-carry primitive
carry_mul<K>, in the manner of tests/test_pair_sqr_model.py.  The model works on 32-bit two's
complement words as the device does, so a limb that does not fit is a wrong value here too.
It also re-derives the column bounds of the product leaves for the closed range [-8, 2^29 + 8]
of a carried limb (carry_mul<12> reaches 2^29 + 8 exactly)."""
import itertools
import random

import pytest

M29 = (1 << 29) - 1
LIMB_MIN, LIMB_MAX = -8, (1 << 29) + 8
TOP = 1 << 17  # |signed top limb| of a value below 2^12.6 p


def s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def value(limbs):
    return sum(v << (29 * k) for k, v in enumerate(limbs))


def pair_carry(limbs):
    """one parallel carry round on 32-bit words (pair_carry); the top limb keeps everything above"""
    w = [s32(x) for x in limbs]
    c = [x >> 29 for x in w]
    out = [(w[0] & M29)] + [(w[k] & M29) + c[k - 1] for k in range(1, 13)] + [w[13] + c[12]]
    return [s32(x) for x in out]


def carry_mul(limbs, K):
    """fps_t::carry_mul<K>: t = m limb, low 29 - s bits shifted up by s, plus the carry t >> (29 - s)"""
    m = 3 if K % 3 == 0 else 1
    s = (K // m).bit_length() - 1
    assert m << s == K
    sh = 29 - s
    t = [s32(s32(x) * m) for x in limbs]
    c = [x >> sh for x in t]
    low = [((x & ((1 << sh) - 1)) << s) for x in t]
    out = [low[0]] + [low[k] + c[k - 1] for k in range(1, 13)] + [s32((t[13] << s)) + c[12]]
    return [s32(x) for x in out]


def carried_vectors(rng, count):
    """carried limb vectors at the corners of [LIMB_MIN, LIMB_MAX], alternating, and random"""
    vs = [[lo] * 13 + [top] for lo, top in itertools.product((LIMB_MIN, LIMB_MAX, 0, M29), (TOP, -TOP, 0))]
    vs += [[LIMB_MAX if k % 2 else LIMB_MIN for k in range(13)] + [TOP],
           [LIMB_MIN if k % 2 else LIMB_MAX for k in range(13)] + [-TOP]]
    vs += [[rng.randrange(LIMB_MIN, LIMB_MAX + 1) for _ in range(13)] + [rng.randrange(-TOP, TOP + 1)] for _ in range(count)]
    return vs


def lazy_sum(plus, minus):
    """the uncarried limb vector of sum(plus) - sum(minus), in 32-bit words, and its exact limbs"""
    exact = [sum(v[k] for v in plus) - sum(v[k] for v in minus) for k in range(14)]
    return [s32(x) for x in exact], exact


def check_carried(limbs):
    assert all(LIMB_MIN <= x <= LIMB_MAX for x in limbs[:13]), limbs


def test_grouped_carry_at_the_limit():
    rng = random.Random(2910)
    vs = carried_vectors(rng, 40)
    hi, lo = [LIMB_MAX] * 13 + [TOP], [LIMB_MIN] * 13 + [-TOP]
    groups = [([hi] * 3, [lo] * 3), ([lo] * 3, [hi] * 3), ([hi, lo, hi], [lo, hi, lo])]
    groups += [(rng.sample(vs, 3), rng.sample(vs, 3)) for _ in range(300)]
    for plus, minus in groups:
        words, exact = lazy_sum(plus, minus)
        assert words == exact  # P = 3, N = 3: no limb wraps
        out = pair_carry(words)
        assert value(out) == value(exact)
        check_carried(out)
    # one more term does not fit: the static_assert's reason
    words, exact = lazy_sum([hi] * 4, [])
    assert words != exact
    words, exact = lazy_sum([], [hi] * 4)
    assert words != exact


# (K, P, N) at the limits fps_carry_mul_ok admits
ADMITTED = [(2, 3, 3), (4, 3, 1), (8, 2, 0), (3, 1, 0), (3, 0, 1), (12, 1, 0)]


@pytest.mark.parametrize("K,P,N", ADMITTED)
def test_small_multiple_with_carry(K, P, N):
    rng = random.Random(K * 100 + P * 10 + N)
    vs = carried_vectors(rng, 40)
    hi, lo = [LIMB_MAX] * 13 + [TOP], [LIMB_MIN] * 13 + [-TOP]
    groups = [([hi] * P, [lo] * N), ([lo] * P, [hi] * N)]
    groups += [([rng.choice(vs) for _ in range(P)], [rng.choice(vs) for _ in range(N)]) for _ in range(300)]
    for plus, minus in groups:
        words, exact = lazy_sum(plus, minus)
        assert words == exact
        out = carry_mul(words, K)
        assert value(out) == K * value(exact)
        check_carried(out)
    # the ends of the sum's range beside a limb whose low part is empty or full
    m = 3 if K % 3 == 0 else 1
    sh = 29 - ((K // m).bit_length() - 1)
    full = next(x for x in (((j << sh) - 1) // m for j in range(1, 4)) if (m * x + 1) % (1 << sh) == 0)
    assert 0 < full <= LIMB_MAX
    for end in (P * LIMB_MAX - N * LIMB_MIN, P * LIMB_MIN - N * LIMB_MAX):
        for filler in (0, full) if P else (0,):
            exact = [end, filler] * 6 + [end, 0]
            out = carry_mul([s32(x) for x in exact], K)
            assert value(out) == K * value(exact)
            check_carried(out)


def test_carry_mul_reaches_the_closed_upper_end():
    # 3 x = 2^28 - 1 leaves the low part 2^29 - 4, and the limb 2^29 below it carries 12
    x = ((1 << 28) - 1) // 3
    limbs = [1 << 29, x] * 6 + [1 << 29, 0]
    out = carry_mul(limbs, 12)
    assert value(out) == 12 * value(limbs) and max(out[:13]) == LIMB_MAX


@pytest.mark.parametrize("K,P,N", [(4, 1, 2), (8, 1, 1), (8, 3, 0), (12, 2, 0), (12, 0, 1), (3, 2, 0)])
def test_rejected_small_multiples_do_leave_the_range(K, P, N):
    # a limb at an end of the sum's range beside one whose low part is empty or full
    m = 3 if K % 3 == 0 else 1
    sh = 29 - ((K // m).bit_length() - 1)
    ends = (P * LIMB_MAX - N * LIMB_MIN, P * LIMB_MIN - N * LIMB_MAX)
    bad = 0
    for end, filler in itertools.product(ends, (0, (1 << sh) - 1 if m == 1 else 0)):
        exact = [end, filler] * 6 + [end, 0]
        out = carry_mul([s32(x) for x in exact], K)
        if value(out) != K * value(exact) or not all(LIMB_MIN <= x <= LIMB_MAX for x in out[:13]):
            bad += 1
    assert bad


def test_column_bounds_of_the_leaves_for_the_closed_range():
    """|t| < 2^63 for the 64-bit accumulators with operand limbs in [-8, 2^29 + 8]: per lane a
    column takes 7 steps of product terms and one reduction term m p_j < 2^29 2^29 each, plus
    carries below 2^35 that stay behind (lsg_fp_pair.hpp, comments of the three passes)"""
    L = LIMB_MAX
    red = (1 << 29) * (1 << 29)
    stay = 1 << 35
    assert 7 * (L * L + red) + stay < 1 << 63                  # pair_mont_mul_n
    assert 7 * (2 * L * (L + 8) + red) + stay < 1 << 63        # ... (a0 + a1)(a0 - a1) of the Fp2 squaring leaf
    assert 7 * (L * (2 * L) + red) + stay < 1 << 63            # pair_mont_sqr_n: the doubled operand
    assert 7 * (2 * L * L + red) + stay < 1 << 63              # pair_sop2_n: two products per step
    # an uncarried sum does not go into pair_sop2_n: with P = 3, N = 3 limbs it would not fit
    U = 3 * L + 3 * 8
    assert 7 * (2 * U * U + red) > 1 << 63
