"""Limb patterns at the lazy bounds of the pair backend (lodestar_amd/csrc/lsg_fp_pair.hpp) for
the squaring-leaf tests: 14 signed radix-2^29 limbs per element, limbs 0..12 in
[-8, 2^29 + 8), a signed top limb, |value| < 2^12.6 p.  The same families as
tests/test_gpu_parity.py::test_device_fp2_leaf_at_lazy_bounds.  Test infrastructure only."""
import itertools
import random

from oracle import hash_to_curve as h2c

P = h2c.P
RINV = pow(1 << 406, -1, P)
BOUND = int(2 ** 12.6 * P)
TOP_MAX = BOUND >> (29 * 13)
HI, LO = (1 << 29) + 7, -8


def value(limbs):
    return sum(v << (29 * k) for k, v in enumerate(limbs))


def clamp(limbs):
    """the top limb's magnitude lowered until |value| < 2^12.6 p"""
    limbs = list(limbs)
    while abs(value(limbs)) >= BOUND:
        limbs[13] += -1 if limbs[13] > 0 else 1
    return limbs


def patterns():
    """16 constant-limb patterns with signed top limbs, 2 alternating extremes, 60 seeded random"""
    pats = [clamp([lo] * 13 + [top]) for lo, top in
            itertools.product((HI, LO, 0, (1 << 29) - 1), (TOP_MAX, -TOP_MAX, 0, 1))]
    pats += [clamp([HI if k % 2 else LO for k in range(13)] + [TOP_MAX]),
             clamp([LO if k % 2 else HI for k in range(13)] + [-TOP_MAX])]
    r = random.Random(77)
    pats += [clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-TOP_MAX, TOP_MAX + 1)])
             for _ in range(60)]
    return pats


def fp2_items():
    """4 n pairs (a0, a1) that walk the patterns at two strides"""
    pats = patterns()
    n = len(pats)
    return [(pats[k % n], pats[(3 * k + 1) % n]) for k in range(4 * n)]


def fp_items():
    """4 n elements: every pattern, then limb-wise mixes of two patterns (even limbs of one, odd
    limbs of the other), which put the extremes of one beside the other's in every column"""
    pats = patterns()
    n = len(pats)
    out = list(pats)
    for k in range(n, 4 * n):
        x, y = pats[k % n], pats[(5 * k + 2) % n]
        out.append(clamp([x[j] if j % 2 else y[j] for j in range(14)]))
    return out


def pair_words(limbs):
    """pair layout of one element: limb L at word 2 (L mod 7) + L / 7"""
    w = [0] * 14
    for L, v in enumerate(limbs):
        w[2 * (L % 7) + L // 7] = v & 0xFFFFFFFF
    return w


def from_pair_words(w):
    limbs = [w[2 * (L % 7) + L // 7] for L in range(14)]
    return [x - (1 << 32) if x >= (1 << 31) else x for x in limbs]
