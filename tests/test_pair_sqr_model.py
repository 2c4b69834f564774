"""The two-lane schedule of the Montgomery squaring pass (lodestar_amd/csrc/lsg_fp_pair.hpp,
pair_mont_sqr_n at LSG_PAIR_G = 2) on Python integers: positions, the hand-down of lane 1's
low 29 bits, the carry that stays behind, and pair_redc_tail.  No GPU and no compiler: this is
the CPU check of the cross-lane schedule (the one-lane host build has no second lane).

At the lazy bounds of the inputs it asserts that
- every column is complete when it is reduced (each a_x a_y with x + y = c has been added with
  its full factor by step c, and the m of every step is the product pass's m),
- no 64-bit accumulator leaves (-2^63, 2^63),
- the output equals the model of pair_mont_mul_n(a, a) limb for limb, and is a^2 / 2^406 mod p
  with limbs 0..12 in [0, 2^29)."""
import random

from tests import sqr_patterns as sp

M29 = (1 << 29) - 1
P_LIMBS = [(sp.P >> (29 * k)) & M29 for k in range(14)]
N0P = (-pow(sp.P, -1, 1 << 29)) % (1 << 29)
LIM = 1 << 63


def _check_range(t):
    for lane in t:
        for v in lane:
            assert -LIM < v < LIM, v


def cios(a, square):
    """One CIOS pass of the pair layout; returns (limbs, m sequence).  square: the i <= s mod 7
    schedule with the doubled broadcast; else the full product a * a."""
    A = [a[0:7], a[7:14]]
    t = [[0] * 7, [0] * 7]
    terms = {}  # column -> {(x, y): factor} of the product terms added so far
    ms = []
    for s in range(14):
        b = a[s]
        for h in range(2):
            if square:
                lim = s % 7
                sched = [(i, 2 * b, 2) for i in range(lim)] + [(lim, b, 1)]
            else:
                sched = [(i, b, 1) for i in range(7)]
            for i, operand, factor in sched:
                assert -(1 << 31) <= operand < (1 << 31)  # the mad's signed 32-bit operand
                t[h][i] += A[h][i] * operand
                col = s + i + 7 * h  # the column position i of lane h holds at step s
                x, y = sorted((s, i + 7 * h))
                assert x + y == col
                d = terms.setdefault(col, {})
                d[(x, y)] = d.get((x, y), 0) + factor
        _check_range(t)
        if square:  # column s is complete: every pair once, doubled off the diagonal
            want = {(x, s - x): (1 if 2 * x == s else 2) for x in range(max(0, s - 13), s // 2 + 1)}
            assert terms.get(s, {}) == want, (s, terms.get(s), want)
        m = ((t[0][0] & 0xFFFFFFFF) * N0P) & M29  # lane 0's, broadcast to the pair
        ms.append(m)
        for h in range(2):
            for j in range(7):
                t[h][j] += m * P_LIMBS[7 * h + j]
        _check_range(t)
        assert t[0][0] & M29 == 0
        down = t[1][0] & M29  # lane 1's low 29 bits move to lane 0's top position
        for h in range(2):
            c = t[h][0] >> 29  # the carry stays in its lane
            t[h] = t[h][1:] + [down if h == 0 else 0]
            t[h][0] += c
        _check_range(t)
    if square:  # the later columns were complete too, and nothing else was added
        for c in range(14, 27):
            want = {(x, c - x): (1 if 2 * x == c else 2) for x in range(c - 13, c // 2 + 1)}
            assert terms[c] == want, c
        assert sorted(terms) == list(range(27))
    # pair_redc_tail
    for h in range(2):
        for j in range(6):
            t[h][j + 1] += t[h][j] >> 29
            t[h][j] &= M29
    ct = t[0][6] >> 29
    t[0][6] &= M29
    t[1][0] += ct
    _check_range(t)
    out = []
    for h in range(2):
        c = t[h][0] >> 29
        r = [t[h][0] & M29]
        for j in range(1, 7):
            v = t[h][j] + c
            if j < 6:
                c = v >> 29
                r.append(v & M29)
            else:
                r.append(v)
        out += r
    return out, ms


def check(a):
    sq, m_sq = cios(a, True)
    mu, m_mu = cios(a, False)
    assert m_sq == m_mu
    assert sq == mu
    va = sp.value(a)
    assert (sp.value(sq) - va * va * sp.RINV) % sp.P == 0
    assert all(0 <= v < (1 << 29) for v in sq[:13])
    assert -(1 << 31) <= sq[13] < (1 << 31)


def test_extreme_patterns():
    for a in sp.fp_items():
        check(a)


def test_all_limbs_at_one_extreme():
    """every limb, the top one included, at the edge of a signed 29-bit-plus-slack word: beyond
    the value bound of a field element, the worst case for the accumulators"""
    for lo in (sp.HI, sp.LO):
        for top in (sp.HI, sp.LO, sp.TOP_MAX, -sp.TOP_MAX):
            a = [lo] * 13 + [top]
            sq, m_sq = cios(a, True)
            mu, m_mu = cios(a, False)
            assert (sq, m_sq) == (mu, m_mu)


def test_random_patterns():
    r = random.Random(2909)
    for _ in range(300):
        check(sp.clamp([r.randrange(sp.LO, sp.HI + 1) for _ in range(13)] +
                       [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)]))
