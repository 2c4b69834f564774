"""The Fp2 layout with one component per lane (lodestar_amd/csrc/lsg_fp2_lanes.hpp) on Python
integers: two lanes, the swaps between them explicit.  The even lane (0) holds the 14 limbs of
c0, the odd lane (1) those of c1; each lane runs a whole 14-column CIOS pass,
  product  REDC(P b_own + Q b_other), P = a0 on both lanes, Q = -a1 on lane 0 and a1 on lane 1
  square   lane 0 REDC((a0 + a1)(a0 - a1)), lane 1 REDC(a1 (2 a0))
with the accumulators carried once after step 7.  No GPU and no compiler.

At the limb extremes of the operands (every limb at -8 or 2^29 + 8, the signed top limb at both
ends of its range, which makes the square's operands the uncarried extremes) it asserts that
- every mad operand fits a signed 32-bit word and no 64-bit accumulator leaves (-2^63, 2^63)
  after any term of any step,
- the m of every step is the Montgomery digit of the integer being reduced,
- lane 0 returns (a0 b0 - a1 b1) / 2^406 and lane 1 (a0 b1 + a1 b0) / 2^406 mod p (the square:
  a0^2 - a1^2 and 2 a0 a1), with limbs 0..12 in [0, 2^29),
- the conversions from and to the pair layout (lane h holds limbs 7h..7h+6 of both components)
  move every limb to the lane the passes read it from, and back."""
import itertools
import random

from tests import sqr_patterns as sp

M29 = (1 << 29) - 1
P_LIMBS = [(sp.P >> (29 * k)) & M29 for k in range(14)]
N0P = (-pow(sp.P, -1, 1 << 29)) % (1 << 29)
R = 1 << 406
LIM = 1 << 63
LO, HI = -8, (1 << 29) + 8  # the closed range of a carried limb


def _in_range(t):
    assert all(-LIM < v < LIM for v in t), t


def _s32(v):
    assert -(1 << 31) <= v < (1 << 31), v
    return v


def swap(x):
    """quad_perm [1, 0, 3, 2] on the two lanes of a pair: every lane gets its partner's word"""
    return [x[1], x[0]]


def reduce_step(t, i, ms):
    m = ((t[0] & 0xFFFFFFFF) * N0P) & M29
    ms.append(m)
    for j in range(14):
        t[j] += m * P_LIMBS[j]
    _in_range(t)
    assert t[0] & M29 == 0
    c = t[0] >> 29
    t[:] = t[1:] + [0]
    t[0] += c
    _in_range(t)
    if i == 6:  # the mid-loop carry
        carry64(t)


def carry64(t):
    for j in range(13):
        t[j + 1] += t[j] >> 29
        t[j] &= M29
    _in_range(t)


def digits(x):
    """the m sequence of REDC(x): the 29-bit digits of -x / p mod 2^406"""
    M = (-x * pow(sp.P, -1, R)) % R
    return [(M >> (29 * i)) & M29 for i in range(14)]


def lanes_mul(a, b):
    """a, b: (c0 limbs, c1 limbs) = what lanes 0 and 1 hold.  Returns the two lanes' results."""
    out = []
    part = [[swap([a[0][k], a[1][k]])[lane] for k in range(14)] for lane in range(2)]  # the partner's a
    for lane in range(2):
        own = a[lane]
        P = part[lane] if lane else own                       # a0 on both lanes
        Q = own if lane else [-x for x in part[lane]]        # -a1 | a1
        assert P == a[0] and Q == ([-x for x in a[1]], a[1])[lane]
        t, ms = [0] * 14, []
        for i in range(14):
            bo = _s32(b[lane][i])
            bs = _s32(swap([b[0][i], b[1][i]])[lane])
            for j in range(14):
                t[j] += _s32(P[j]) * bo
            _in_range(t)
            for j in range(14):
                t[j] += _s32(Q[j]) * bs
            _in_range(t)
            reduce_step(t, i, ms)
        carry64(t)
        out.append((t, ms))
    return out


def lanes_sqr(a):
    out = []
    for lane in range(2):
        own = a[lane]
        part = [swap([a[0][k], a[1][k]])[lane] for k in range(14)]
        V = own if lane else [x + y for x, y in zip(own, part)]          # a0 + a1 | a1
        s = [2 * y for y in part] if lane else [x - y for x, y in zip(own, part)]  # a0 - a1 | 2 a0
        t, ms = [0] * 14, []
        for i in range(14):
            si = _s32(s[i])
            for j in range(14):
                t[j] += _s32(V[j]) * si
            _in_range(t)
            reduce_step(t, i, ms)
        carry64(t)
        out.append((t, ms))
    return out


def check_out(res, want):
    for (t, ms), x in zip(res, want):
        assert ms == digits(x)
        assert all(0 <= v < (1 << 29) for v in t[:13]) and -(1 << 31) <= t[13] < (1 << 31)
        assert sp.value(t) * R == x + sum(m << (29 * i) for i, m in enumerate(ms)) * sp.P  # the exact integer
        assert (sp.value(t) - x * sp.RINV) % sp.P == 0


def check_mul(a, b):
    a0, a1, b0, b1 = (sp.value(x) for x in (*a, *b))
    check_out(lanes_mul(a, b), [a0 * b0 - a1 * b1, a0 * b1 + a1 * b0])


def check_sqr(a):
    a0, a1 = sp.value(a[0]), sp.value(a[1])
    check_out(lanes_sqr(a), [(a0 + a1) * (a0 - a1), 2 * a0 * a1])


def extremes():
    """every low limb at one end of the carried range; the top limb at both ends of the value
    bound, and -- beyond a field element's value, the accumulators' worst case -- at the ends of
    the limb range too"""
    tops = (sp.TOP_MAX, -sp.TOP_MAX, HI, LO)
    pats = [[lo] * 13 + [top] for lo, top in itertools.product((HI, LO), tops)]
    pats += [[HI if k % 2 else LO for k in range(13)] + [sp.TOP_MAX], [LO if k % 2 else HI for k in range(13)] + [-sp.TOP_MAX]]
    return pats


def test_product_at_the_limb_extremes():
    E = extremes()
    for a0, a1 in itertools.product(E, E):
        for b in ((a0, a1), (a1, a0), (E[0], E[5]), (E[5], E[0])):
            check_mul((a0, a1), b)


def test_square_at_the_limb_extremes():
    """the operands a0 + a1, a0 - a1 and 2 a0 enter uncarried: limbs up to 2^30 + 16"""
    E = extremes()
    for a0, a1 in itertools.product(E, E):
        check_sqr((a0, a1))
    V = [x + y for x, y in zip(E[0], E[0])]
    assert max(V[:13]) == (1 << 30) + 16


def test_patterns_and_random():
    items = sp.fp2_items()
    for k, a in enumerate(items[:160]):
        check_mul(a, items[(7 * k + 3) % len(items)])
        check_sqr(a)
    r = random.Random(4051)

    def rnd():
        return sp.clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)])
    for _ in range(100):
        a, b = (rnd(), rnd()), (rnd(), rnd())
        check_mul(a, b)
        check_sqr(a)


def test_lane_assignment_is_not_symmetric():
    """which lane holds which component matters: with the lanes exchanged the product's lane 0
    would return a1 b1 - a0 b0"""
    items = sp.fp2_items()
    a, b = items[5], items[11]
    (t0, _), (t1, _) = lanes_mul(a, b)
    (u0, _), _ = lanes_mul((a[1], a[0]), (b[1], b[0]))
    assert (sp.value(t0) + sp.value(u0)) % sp.P == 0 and sp.value(t0) % sp.P != 0
    assert (sp.value(t1) - (sp.value(a[0]) * sp.value(b[1]) + sp.value(a[1]) * sp.value(b[0])) * sp.RINV) % sp.P == 0


def to_lanes(c0, c1):
    """fp2v_from_pair: lane h of the pair layout holds limbs 7h..7h+6 of c0 and of c1; each lane
    sends the 7 words its partner lacks in one swap per word"""
    pair = [(c0[0:7], c1[0:7]), (c0[7:14], c1[7:14])]  # lane -> (its c0 words, its c1 words)
    lanes = [[None] * 14, [None] * 14]
    for k in range(7):
        s = swap([pair[0][1][k], pair[1][0][k]])  # lane 0 sends its c1 word, lane 1 its c0 word
        lanes[0][k], lanes[0][7 + k] = pair[0][0][k], s[0]
        lanes[1][k], lanes[1][7 + k] = s[1], pair[1][1][k]
    return lanes


def from_lanes(lanes):
    pair = [([None] * 7, [None] * 7), ([None] * 7, [None] * 7)]
    for k in range(7):
        s = swap([lanes[0][7 + k], lanes[1][k]])  # lane 0 sends limb 7 + k of c0, lane 1 limb k of c1
        pair[0][0][k], pair[0][1][k] = lanes[0][k], s[0]
        pair[1][0][k], pair[1][1][k] = s[1], lanes[1][7 + k]
    return pair[0][0] + pair[1][0], pair[0][1] + pair[1][1]


def test_conversions_put_c0_on_the_even_lane():
    c0, c1 = list(range(100, 114)), list(range(200, 214))
    lanes = to_lanes(c0, c1)
    assert lanes == [c0, c1]
    assert from_lanes(lanes) == (c0, c1)
