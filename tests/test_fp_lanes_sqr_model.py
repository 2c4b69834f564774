"""The triangular squaring pass of the one-element-per-lane powers (lodestar_amd/csrc/
lsg_fp2_lanes.hpp lanes_sqr_pass) on Python integers, beside the product pass it replaces
(lanes_mul_pass, modelled as tests/test_fp2_lanes_model.py models the other passes).  At step i
position j of the accumulators holds column i + j; the step adds a_i a_i at position i and
a_w (2 a_i) at every position w > i, then reduces.  No GPU and no compiler.

For every input it asserts that
- every mad operand fits a signed 32-bit word and no 64-bit accumulator leaves (-2^63, 2^63)
  after any term of any step,
- the m of every step is the Montgomery digit of a^2, and the m sequence equals that of the
  product pass on (a, a),
- the 14 result words equal the product pass's, are a^2 / 2^406 mod p exactly, with limbs 0..12
  in [0, 2^29).
Inputs: the limb extremes (every low limb at -8 or 2^29 + 8, the top limb at both ends), the
patterns of tests/sqr_patterns.py, the edge values of tests/field_edges.py in every lazy
representation, random values."""
import random

from tests import field_edges as fe
from tests import sqr_patterns as sp
from tests.test_fp2_lanes_model import HI, LO, _in_range, _s32, carry64, digits, extremes, reduce_step, R


def mul_pass(V, s):
    """lanes_mul_pass: REDC(V s)"""
    t, ms = [0] * 14, []
    for i in range(14):
        si = _s32(s[i])
        for j in range(14):
            t[j] += _s32(V[j]) * si
        _in_range(t)
        reduce_step(t, i, ms)
    carry64(t)
    return t, ms


def sqr_pass(a):
    """lanes_sqr_pass: REDC(a a), each cross product once"""
    t, ms = [0] * 14, []
    mads = 0
    for i in range(14):
        ai, di = _s32(a[i]), _s32(2 * a[i])
        t[i] += _s32(a[i]) * ai
        _in_range(t)
        for w in range(i + 1, 14):
            t[w] += _s32(a[w]) * di
            _in_range(t)
        mads += 14 - i
        reduce_step(t, i, ms)
    carry64(t)
    assert mads == 105
    return t, ms


def check(a):
    x = sp.value(a) ** 2
    t, ms = sqr_pass(a)
    tm, mm = mul_pass(a, a)
    assert ms == mm == digits(x)
    assert t == tm
    assert all(0 <= v < (1 << 29) for v in t[:13]) and -(1 << 31) <= t[13] < (1 << 31)
    assert sp.value(t) * R == x + sum(m << (29 * i) for i, m in enumerate(ms)) * sp.P  # the exact integer
    assert (sp.value(t) - x * sp.RINV) % sp.P == 0


def test_square_at_the_limb_extremes():
    for a in extremes():
        check(a)
    assert max(2 * v for v in extremes()[0][:13]) == (1 << 30) + 16  # the doubled operand, uncarried


def test_patterns():
    for a in sp.fp_items():
        check(a)


def test_edge_values_in_every_lazy_representation():
    n = 0
    for v, _ in fe.canon_values():
        for e in fe.E_VECTORS.values():
            check(fe.rep(v, e))
            n += 1
    assert n > 0


def test_random():
    r = random.Random(1709)
    for _ in range(300):
        check(sp.clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)]))
