"""The lazy sums of the pair backend on the device (lodestar_amd/csrc/lsg_fp_pair.hpp fps_t,
lsg_tower.hpp fp2s_t): lsg_check_sums runs, over the limb patterns of tests/sqr_patterns.py (312
items: full waves and a partial one), the maximal admissible chain, the small multiples,
fp2_mul_b3, a Jacobian doubling over Fp and over Fp2, the complete G2 addition and the longest
combination of the fused Miller kernel, each beside the form that carries at every operation,
evaluated in the same kernel.  Results without a product are compared with Python integers
exactly; the others are congruent mod p to the formula and equal, as integers, to the nested
form.  Then the shipped path at the shapes where the fused Miller kernel can go wrong.
Every test here needs an MI355X."""
import hashlib

import pytest

from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu
P, RINV = sp.P, sp.RINV
EIN, EOUT = 12, 42
LIMB_MIN, LIMB_MAX = -8, (1 << 29) + 8


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def run(ctx):
    """(ring of input limb vectors, per item the 42 output limb vectors)"""
    fp = sp.fp_items()
    n = len(fp)
    assert n == 312
    ring = [fp[(i + 29 * j) % n] for i in range(n) for j in range(EIN)]
    out = ctx.check_sums([w for e in ring for w in sp.pair_words(e)])
    assert len(out) == 14 * EOUT * n
    rows = [[sp.from_pair_words(out[14 * (EOUT * i + k):14 * (EOUT * i + k) + 14]) for k in range(EOUT)] for i in range(n)]
    return ring, rows


def els(ring, i, count):
    return [sp.value(ring[(EIN * i + j) % len(ring)]) for j in range(count)]


def carried(limbs):
    return all(LIMB_MIN <= x <= LIMB_MAX for x in limbs[:13])


def test_sums_and_small_multiples_are_exact(run):
    ring, rows = run
    for i, row in enumerate(rows):
        a, b, c, d, e, f = els(ring, i, 6)
        want = [a + b + c - d - e - f, 2 * a, 3 * a, 4 * a, 8 * a, 12 * a, 12 * (a - b), 12 * (a + b)]
        assert [sp.value(v) for v in row[:8]] == want, i
        assert all(carried(v) for v in row[:8]), i


# ---- the formulas on Montgomery residues: mul(x, y) = x y / 2^406
def f_mul(x, y):
    return x * y * RINV % P


def f2_mul(x, y):
    return (f_mul(x[0], y[0]) - f_mul(x[1], y[1]), f_mul(x[0], y[1]) + f_mul(x[1], y[0]))


def f2(op):
    return lambda x, y: (op(x[0], y[0]), op(x[1], y[1]))


class Fp1:
    mul = staticmethod(f_mul)
    add = staticmethod(lambda x, y: x + y)
    sub = staticmethod(lambda x, y: x - y)
    k = staticmethod(lambda c, x: c * x)
    b3 = staticmethod(lambda x: 12 * x)
    eq = staticmethod(lambda x, y: (x - y) % P == 0)


class Fp2:
    mul = staticmethod(f2_mul)
    add = staticmethod(f2(lambda x, y: x + y))
    sub = staticmethod(f2(lambda x, y: x - y))
    k = staticmethod(lambda c, x: (c * x[0], c * x[1]))
    b3 = staticmethod(lambda x: (12 * (x[0] - x[1]), 12 * (x[0] + x[1])))
    eq = staticmethod(lambda x, y: (x[0] - y[0]) % P == 0 and (x[1] - y[1]) % P == 0)


def jac_dbl(F, X, Y, Z):
    A, B = F.mul(X, X), F.mul(Y, Y)
    C = F.mul(B, B)
    s = F.add(X, B)
    D = F.k(2, F.sub(F.sub(F.mul(s, s), A), C))
    E = F.k(3, A)
    X3 = F.sub(F.mul(E, E), F.k(2, D))
    return X3, F.sub(F.mul(E, F.sub(D, X3)), F.k(8, C)), F.k(2, F.mul(Y, Z))


def proj_add(F, p, q):
    """RCB 2016 algorithm 7, a = 0"""
    t0, t1, t2 = F.mul(p[0], q[0]), F.mul(p[1], q[1]), F.mul(p[2], q[2])
    t3 = F.sub(F.mul(F.add(p[0], p[1]), F.add(q[0], q[1])), F.add(t0, t1))
    t4 = F.sub(F.mul(F.add(p[1], p[2]), F.add(q[1], q[2])), F.add(t1, t2))
    Y3 = F.sub(F.mul(F.add(p[0], p[2]), F.add(q[0], q[2])), F.add(t0, t2))
    t0 = F.k(3, t0)
    t2 = F.b3(t2)
    Z3, t1 = F.add(t1, t2), F.sub(t1, t2)
    Y3 = F.b3(Y3)
    X3 = F.sub(F.mul(t3, t1), F.mul(t4, Y3))
    return X3, F.add(F.mul(t1, Z3), F.mul(Y3, t0)), F.add(F.mul(Z3, t4), F.mul(t0, t3))


def test_doublings_and_addition_match_formula_and_nested_form(run):
    ring, rows = run
    for i, row in enumerate(rows):
        v = [sp.value(x) for x in row]
        e = els(ring, i, 12)
        # the lazy form and the nested form evaluated beside it: the same integers
        assert v[8:11] == v[11:14] and v[14:20] == v[20:26] and v[26:32] == v[32:38], i
        want = jac_dbl(Fp1, e[0], e[1], e[2])
        assert all(Fp1.eq(v[8 + k], want[k]) for k in range(3)), i
        pairs = [(e[2 * k], e[2 * k + 1]) for k in range(6)]
        want = jac_dbl(Fp2, *pairs[:3])
        assert all(Fp2.eq((v[14 + 2 * k], v[15 + 2 * k]), want[k]) for k in range(3)), i
        want = proj_add(Fp2, pairs[:3], pairs[3:])
        assert all(Fp2.eq((v[26 + 2 * k], v[27 + 2 * k]), want[k]) for k in range(3)), i
        assert all(carried(x) for x in row[8:38]), i


def test_fused_kernel_combination_is_exact(run):
    """t2_0 - t0_0 - xi n2 of the M phase = V11 - V0 + xi (V15 - V12 - V13 - V4 + V1 + V2 - V7 - V9)"""
    ring, rows = run
    for i, row in enumerate(rows):
        e = els(ring, i, 32)
        V = [(e[2 * k], e[2 * k + 1]) for k in range(16)]
        inner = [V[15][c] - V[12][c] - V[13][c] - V[4][c] + V[1][c] + V[2][c] - V[7][c] - V[9][c] for c in range(2)]
        want = [V[11][0] - V[0][0] + inner[0] - inner[1], V[11][1] - V[0][1] + inner[0] + inner[1]]
        assert [sp.value(x) for x in row[38:40]] == want, i
        assert [sp.value(x) for x in row[40:42]] == want, i
        assert carried(row[38]) and carried(row[39]), i


# ---- the shipped path: packages of single-key sets at the fused kernel's shapes
N_KEYS = 129


@pytest.fixture(scope="module")
def sets(ctx):
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    msgs = [hashlib.sha256(b"lodestar-mi355x" + b"lazy-sums" + i.to_bytes(8, "little")).digest() for i in range(N_KEYS)]
    return [([pks[i]], msgs[i], s) for i, s in enumerate(ctx.sign(sks, msgs))]


def _splitmix(seed, n):
    M = (1 << 64) - 1
    s, out = seed, []
    while len(out) < n:
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        if z:
            out.append(z)
    return out


@pytest.mark.parametrize("wrong", [False, True])
@pytest.mark.parametrize("n", [1, 4, 5, 33, 129])
def test_shipped_package_partial_and_verdicts(ctx, sets, n, wrong):
    """One pair in an item (1), a full item (4), a full item plus a one-pair item (5), a full wave
    of items plus one (33), a full 128-set workgroup plus one (129): lsg_jobs_partial equals the
    oracle's partial byte for byte and the per-job verdicts are the C oracle's, valid and with one
    wrong message (on the last set: the partial item, wave or workgroup)."""
    from oracle import verifier as ov
    from oracle.fields import f12_coeffs, f12_pow
    ss = list(sets[:n])
    if wrong:
        ss[n - 1] = bd.corrupt_wrong_message(ss[n - 1])
    seed = 0x50a50000 + 2 * n + int(wrong)
    t = ctx.submit_jobs([([s], 1) for s in ss], seed=seed)
    part, has = ctx.jobs_partial(t)
    assert has
    flat = [(p[0], m, s) for p, m, s in ss]
    if n == 1:
        exp, errs = ov.batch_partial(flat, [1])
        exp = f12_pow(exp, _splitmix(seed ^ 0x5851F42D4C957F2D, 1)[0])
    else:
        exp, errs = ov.batch_partial(flat, _splitmix(seed, n))
    assert errs == [0] * n
    want = b"".join(int(c[0]).to_bytes(48, "big") + int(c[1]).to_bytes(48, "big") for c in f12_coeffs(exp))
    assert part == want
    per = co.verify_each([p[0] for p, _, _ in ss], [m for _, m, _ in ss], [s for _, _, s in ss])
    assert per == [1] * (n - 1) + [0 if wrong else 1]
    assert ctx.wait_jobs(t)[0] == [(1, 0) if ok else (0, 0) for ok in per]
