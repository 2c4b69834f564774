"""Case tables for the layer between the Montgomery products and the accept / reject rules of
the pair backend (lodestar_amd/csrc/lsg_fp_pair.hpp, lsg_tower.hpp, lsg_inv.hpp, lsg_h2c.hpp):
canonical forms and the predicates on them, byte conversions, Fp2 roots and signs, the two
inversions, the batched inversion's zero handling and the map from chosen "uniform bytes".
Plain Python: inputs and expected values only, the latter from Python integers and oracle/.
tests/test_field_edges_host.py runs the tables through the one-lane host build of the headers,
tests/test_gpu_field_edges.py through the device hooks.  Test infrastructure only."""
import functools
import random

from oracle import hash_to_curve as h2c
from oracle.curves import E2, g2_serialize
from oracle.fields import P, f2_sqr, f2_sqrt, f2_sgn0, f2_lexi_largest

R = 1 << 406
RINV = pow(R, -1, P)
R2 = (1 << 812) % P
HALF_LO, HALF_HI = (P - 1) // 2, (P + 1) // 2
LIMB = 1 << 29


def value(limbs):
    return sum(v << (29 * k) for k, v in enumerate(limbs))


def norm_limbs(v):
    """limbs 0..12 in [0, 2^29), a signed top limb"""
    return [(v >> (29 * k)) & (LIMB - 1) for k in range(13)] + [v >> (29 * 13)]


def _unit(k, s):
    return [s if j == k else 0 for j in range(14)]


# offset vectors e: limbs 0..12 in [-8, 8], top limb 0
E_VECTORS = {
    "zero": [0] * 14,
    "all+8": [8] * 13 + [0],       # zero becomes 2^29, then 2^29 - 1 twelve times, top limb -1
    "all-8": [-8] * 13 + [0],
    "alt": [8 if k % 2 == 0 else -8 for k in range(13)] + [0],
    "l6+8": _unit(6, 8),           # the last limb of the pair's low lane
    "l6-8": _unit(6, -8),
    "l7+8": _unit(7, 8),           # the first limb of its high lane
    "l7-8": _unit(7, -8),
}


def rep(v, e):
    """A lazy representation of the integer v: the normalised limbs of v - value(e), plus e limb
    by limb.  Limbs 0..12 stay in [-8, 2^29 + 8) and the value is exactly v."""
    out = [a + b for a, b in zip(norm_limbs(v - value(e)), e)]
    assert value(out) == v and all(-8 <= x <= LIMB + 8 for x in out[:13])
    return out


def all_reps(v):
    return [rep(v, e) for e in E_VECTORS.values()]


# ---- pair_canon / fp_is_zero: any lazy value
def canon_values():
    out = []
    for k in (0, 1, -1, 2, -2, 3, -3, 4095, -4095):
        for d in (0, 1, -1, HALF_LO, HALF_HI):
            v = k * P + d
            if abs(v) < (P << 12):
                out.append((v, d == 0))
    return out


# ---- fp_canonical, fp_canon_gt_half, fp_canon_parity: values in (-p, 2p)
def canonical_values():
    vs = [-P + 1, -1, 0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P - 1]
    for h in (HALF_LO - 1, HALF_LO, HALF_HI, HALF_HI + 1):
        vs += [h, h + P, h - P]
    for j in range(1, 14):
        vs += [1 << (29 * j), (1 << (29 * j)) - 1]
    vs += [(1 << 203) + 1, (1 << 203) - 1]
    assert all(-P < v < 2 * P for v in vs)
    return vs


# ---- fp_canon_lt_p: raw decoded integers below 2^384
def lt_p_values():
    vs = [0, P - 1, P, P + 1, (1 << 381) - 1, (1 << 384) - 1]
    for k in (0, 28, 29, 202, 203, 204, 376, 380):
        vs += [P + (1 << k), P - (1 << k)]
    assert all(0 <= v < (1 << 384) for v in vs)
    return vs


# ---- fp_from_be_bytes / fp_to_be48
def byte_values():
    return [1 << k for k in range(384)] + [(1 << 384) - 1, P - 1]


# ---- Fp2 roots (canonical (c0, c1); the hooks take them in Montgomery form)
def root_values():
    r = random.Random(20240517)
    vs = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1)]
    for k in range(2, 20):
        vs += [(k, 0), (P - k, 0), (0, k), (0, P - k)]
    for k in range(2, 20):
        vs += [f2_sqr((k, 0)), f2_sqr((0, k)), f2_sqr((k, k)), f2_sqr((k, P - k))]
    vs += [(r.randrange(P), r.randrange(P)) for _ in range(64)]
    vs += [(k, 1) for k in range(1, 25)]
    return vs


def root_expectations(vs):
    """[(a, root or None)] with the counts the table has to reach, from the oracle alone"""
    exp = [(a, f2_sqrt(a)) for a in vs]
    squares = [s for _, s in exp if s is not None]
    assert len(squares) >= 20 and len(exp) - len(squares) >= 20
    assert sum(1 for s in squares if s[0] == 0 or s[1] == 0) >= 10
    return exp


# ---- fp2_sgn0 / fp2_lexi_largest
def sign_values():
    x = random.Random(7).randrange(1, P)
    return [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (0, P - 1), (P - 1, 0), (1, 1), (2, 1),
            (HALF_LO, 0), (HALF_HI, 0), (x, HALF_LO), (x, HALF_HI), (x, 0)]


def sign_expect(a):
    return int(f2_sgn0(a)), bool(f2_lexi_largest(a))


# ---- the inversions: raw integers X; both forms return x with x X = 2^812 (mod p)
def inv_values():
    r = random.Random(99)
    vs = [0, 1, 2, P - 1, P - 2, HALF_LO, HALF_HI]
    for k in range(2, 381):
        vs += [1 << k, (1 << k) - 1]
    return vs + [r.randrange(P) for _ in range(64)]


def inv_ok(x_in, x_out):
    return (x_in * x_out - R2) % P == 0 if x_in % P else x_out % P == 0


# ---- batched inversion
def _zero_reps():
    es = list(E_VECTORS.values())
    return [[0] * 14] + [rep(P, e) for e in es] + [rep(-P, e) for e in es] + [rep(0, e) for e in es[1:]]


def batch_cases(n, chunk, block):
    """[(name, elements)] for a batched inversion of n values: chunk = the values one lane pair
    folds (T), block = the values under one root (128 T in the one-launch form, T in the
    multi-level form).  Non-zero values are lazy representations of seeded random integers
    with |v| < 2^12 p; zeros are written as plain zero and as rep(+-p, e), rep(0, e)."""
    r = random.Random(1000 + n)
    es = list(E_VECTORS.values())
    zs = _zero_reps()

    def nonzero(i):
        v = r.randrange(1, P) + r.randrange(-4095, 4095) * P
        return rep(v, es[i % len(es)])

    base = [nonzero(i) for i in range(n)]
    zero_at = {0, n - 1}
    if chunk > 1 and n >= 3 * chunk:  # both (all) values of one lane pair's chunk
        zero_at |= set(range(chunk, 2 * chunk))
    elif n > 4:
        zero_at |= {2, 3}
    if n >= 2 * block:  # everything under one root
        zero_at |= set(range(block, 2 * block))
    elif n > block:
        zero_at |= set(range(block))
    edges = [zs[i % len(zs)] if i in zero_at else base[i] for i in range(n)]
    cases = [("edges", edges), ("all-zero", [zs[i % len(zs)] for i in range(n)])]
    if n >= 2:  # one zero among non-zero values, whatever the placements above add up to at this n
        cases.append(("first", [zs[n % len(zs)]] + base[1:]))
    return cases


BLOCK_SIZES = (1, 2, 127, 128, 129, 8192, 8193)   # 8193: the first size with T = 2
LEVEL_SIZES = (1, 16, 17, 256, 257, 4097)         # the fold / root / unfold form, T = 16


def block_chunk(n):
    """the T of batch_inv's one-launch form"""
    return min(64, max(1, (n + 128 * 64 - 1) // (128 * 64)))


# ---- the map from uniform bytes
def enc64(n):
    return int(n).to_bytes(64, "big")


def _top_multiple(u):
    return u + ((1 << 512) - 1 - u) // P * P


def _map_specials(r):
    def rnd():
        return (r.randrange(P), r.randrange(P))

    def plain(u0, u1):
        return [u0[0], u0[1], u1[0], u1[1]]

    u, w = rnd(), rnd()
    neg = ((-u[0]) % P, (-u[1]) % P)
    splits = [(1 << 256) - 1, 1 << 256, (1 << 384) - 1, 1 << 384, (1 << 512) - 1]
    return [
        plain((0, 0), rnd()),                     # u0 = 0: the exceptional case of SSWU
        plain(rnd(), (0, 0)),                     # u1 = 0
        plain((0, 0), (0, 0)),                    # both (and a doubling)
        plain(u, u),                              # u1 = u0: a doubling in g2_add
        plain(u, neg),                            # u1 = -u0: the sum is the identity
        [0, 0, P, _top_multiple(0)],              # zero as N = 0, p and the top multiple of p
        plain((0, 1), (0, 2)),                    # sgn0 at the small values
        plain((1, 0), (2, 0)),
        plain((P - 1, 0), (0, P - 1)),
        [w[0], w[1] + P, _top_multiple(w[0]), _top_multiple(w[1])],  # the encodings of one u
        [u[0] + P, _top_multiple(u[1]), neg[0], neg[1] + P],         # ... of u and -u: identity
        splits[:4],                               # the split points of fp_from_be64_mod
        [splits[4], splits[1], splits[3], splits[0]],
    ]


@functools.lru_cache(maxsize=None)
def map_table(n):
    """n items [(256 bytes, expected 192 bytes)]: the special items at index 0, in the middle
    and last, evenly spread between ordinary seeded ones"""
    r = random.Random(4000 + n)
    sp = _map_specials(r)
    at = {round(j * (n - 1) / (len(sp) - 1)): s for j, s in enumerate(sp)}
    assert len(at) == len(sp) and 0 in at and n - 1 in at and (n - 1) // 2 in at
    out = []
    for i in range(n):
        N = at.get(i) or [r.randrange(1 << 512) for _ in range(4)]
        u0, u1 = (N[0] % P, N[1] % P), (N[2] % P, N[3] % P)
        pt = h2c.clear_cofactor(E2.add(h2c.map_to_curve_g2(u0), h2c.map_to_curve_g2(u1)))
        out.append((b"".join(enc64(x) for x in N), g2_serialize(pt)))
    return out


MAP_SIZES = (33, 130)  # a partial wave each; 260 norms make three inversion blocks
