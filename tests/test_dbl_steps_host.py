"""The doubling steps built on squares -- proj_dbl (lodestar_amd/csrc/lsg_curve.hpp: 3 products and
5 squares), ml_dbl_line_sq (lsg_pairing.hpp, the arithmetic of the fused Miller kernel's doubling
step: 2 products and 7 squares) -- and the chains on them (proj_mul_u64_s3, homogeneous throughout
over Fp; the |x| chain with an affine base point and mixed additions) on the CPU, through the
stand-alone driver tests/native/dblcheck.cpp: the one-lane host build of the pair backend, so the
representation, the lazy sums and their bounds are those of the gfx950 build.  Built once plainly
and once with UBSan (a 64-bit column or a 32-bit lazy limb that overflowed would trap) and run
directly.

Every new value is compared (a) with the driver's restatement of the formulas it replaced -- as
field elements, coordinate by coordinate, for the doubling steps: they are the same elements, not
another scaling; as points for the chains -- (b) with the formulas evaluated on Python integers and
(c) with the oracle's group law.  Inputs: random points, the identity (0 : 1 : 0), points with
X = 0 (a point of order 3 on E1; E2 has none, asserted, so X = 0 enters the Fp2 steps as field
values), the non-subgroup points of the golden decode cases (err == 3; the one entry of
mainnet_g2_points_bad.json is not on the curve, which is asserted and why it gives no point),
points of order 13 and 23 on E2 (inside a chain the accumulator meets the identity and +- the
base), and coordinates at the lazy bounds: every offset vector of tests/field_edges.py on
multiples of p up to 2^11 p -- the sum of two coordinates is a product operand, whose bound is
2^12.6 p (lsg_fp_pair.hpp).  Exact comparisons only; a failed compile is an error."""
import json
import os
import random
import shutil
import subprocess

import pytest

from oracle.curves import E1, E2, G1_GEN, G2_GEN, B2, in_g2_psi
from oracle.curves import _Fp, _Fp2
from oracle.fields import P, f2_sqrt
from tests import field_edges as fe
from tests.g2points import decode_on_curve, of_order

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "dblcheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
GOLD = os.path.join(HERE, "golden")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}
R, RINV = fe.R, fe.RINV
X_ABS = 0xd201000000010000
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
S3_SCALARS = [1, 2, 3, 4, 5, 7, 8, 1 << 63, (1 << 64) - 1, 0x4924924924924924, 0xdb6db6db6db6db6d]
EDGE_MULTIPLES = (0, 1, -1, 2047, -2047)


# ---- values
def mont(v, k=0, e=None):
    """limbs of a lazy representation of the Montgomery form of v, plus k p"""
    return fe.rep(v * R % P + k * P, e or fe.E_VECTORS["zero"])


def canon(limbs):
    return fe.value(limbs) * RINV % P


def limbs_of(F, v, k=0, e=None):
    return mont(v, k, e) if F is _Fp else mont(v[0], k, e) + mont(v[1], k, e)


def width(F):
    return 14 if F is _Fp else 28


def take(F, w, i):
    n = width(F)
    c = w[n * i:n * i + n]
    return canon(c) if F is _Fp else (canon(c[:14]), canon(c[14:]))


def to_affine(F, X, Y, Z):
    if F.is_zero(Z):
        return None
    zi = F.inv(Z)
    return (F.mul(X, zi), F.mul(Y, zi))


def b3(F):
    return 12 if F is _Fp else (12, 12)


def small(F, k, a):
    return a * k % P if F is _Fp else (a[0] * k % P, a[1] * k % P)


def alg9(F, X, Y, Z):
    """RCB 2016 algorithm 9 on Python integers"""
    t0 = F.sqr(Y)
    Z3 = small(F, 8, t0)
    t1 = F.mul(Y, Z)
    t2 = F.mul(b3(F), F.sqr(Z))
    X3 = F.mul(t2, Z3)
    Y3 = F.add(t0, t2)
    Z3 = F.mul(t1, Z3)
    t0 = F.sub(t0, small(F, 3, t2))
    Y3 = F.add(X3, F.mul(t0, Y3))
    X3 = small(F, 2, F.mul(t0, F.mul(X, Y)))
    return X3, Y3, Z3, t1, t2


# ---- points
@pytest.fixture(scope="module")
def points():
    rnd = random.Random(2020)
    g1 = [E1.mul(G1_GEN, rnd.randrange(1, R_ORDER)) for _ in range(3)]
    g2 = [E2.mul(G2_GEN, rnd.randrange(1, R_ORDER)) for _ in range(3)]
    x0_1 = (0, 2)  # y^2 = 4: on E1, of order 3
    assert E1.on_curve(x0_1) and E1.mul(x0_1, 3) is None
    assert f2_sqrt(B2) is None  # E2 has no point with x = 0: 4 (1 + u) is no square (X = 0 enters as field values)
    bad = json.load(open(os.path.join(GOLD, "mainnet_g2_points_bad.json")))
    assert all(decode_on_curve(c["sig"]) is None for c in bad)  # not on the curve: no point to chain from
    cases = json.load(open(os.path.join(GOLD, "sig_decode.json")))["cases"]
    non_sub = [decode_on_curve(c["sig"]) for c in cases if c["err"] == 3]
    non_sub = [q for q in non_sub if q is not None]
    assert non_sub and all(E2.on_curve(q) and not in_g2_psi(q) for q in non_sub)
    small_order = [of_order(13, non_sub), of_order(23, non_sub)]
    return {"g1": g1 + [x0_1], "g2": g2 + non_sub[:3] + small_order}


@pytest.fixture(scope="module")
def items(points):
    """[(op, F, input values, input line)]"""
    rnd = random.Random(77)
    es = list(fe.E_VECTORS.values())
    out = []

    def proj_line(F, X, Y, Z, ks=(0, 0, 0), e=None):
        return limbs_of(F, X, ks[0], e) + limbs_of(F, Y, ks[1], e) + limbs_of(F, Z, ks[2], e)

    def fld(F):
        return rnd.randrange(P) if F is _Fp else (rnd.randrange(P), rnd.randrange(P))

    for F, op, key in ((_Fp, "D1", "g1"), (_Fp2, "D2", "g2")):
        pts = [(x, y, F.one) for x, y in points[key]] + [(F.zero, F.one, F.zero)]
        # a point in another projective scaling, and field values that are no point at all
        pts += [tuple(F.mul(c, s) for c in pts[0]) for s in (fld(F),)] + [(fld(F), fld(F), fld(F)) for _ in range(4)]
        # X = 0 (J = 0, 2XY = 0), Y = 0 and Z = 0 as field values: the formulas are compared as field elements
        pts += [(F.zero, fld(F), fld(F)), (F.zero, fld(F), F.one), (fld(F), F.zero, fld(F)), (fld(F), fld(F), F.zero)]
        for X, Y, Z in pts:
            out.append((op, F, (X, Y, Z), proj_line(F, X, Y, Z)))
        X, Y, Z = pts[0]
        for n, e in enumerate(es):  # the lazy bounds: every offset vector, the multiples of p in turn
            for j in range(len(EDGE_MULTIPLES)):
                ks = tuple(EDGE_MULTIPLES[(j + n + c) % len(EDGE_MULTIPLES)] for c in range(3))
                out.append((op, F, (X, Y, Z), proj_line(F, X, Y, Z, ks, e)))
    # the Miller doubling step: T in every form above, P a G1 point
    px, py = points["g1"][0]
    d2 = [it for it in out if it[0] == "D2"]
    for _, _, (X, Y, Z), line in d2:
        out.append(("L2", _Fp2, (X, Y, Z, px, py), line + mont(px) + mont(py)))
    for n, e in enumerate(es):
        k = EDGE_MULTIPLES[n % len(EDGE_MULTIPLES)]
        X, Y, Z = d2[0][2]
        out.append(("L2", _Fp2, (X, Y, Z, px, py), proj_line(_Fp2, X, Y, Z, (k, -k, k), e) + mont(px, k, e) + mont(py, -k, e)))
    # the window chain: every scalar on a random point, the special points on all of them
    for F, op, key in ((_Fp, "S1", "g1"), (_Fp2, "S2", "g2")):
        for n, pt in enumerate(points[key][2:] + [None]):
            X, Y, Z = (pt[0], pt[1], F.one) if pt else (F.zero, F.one, F.zero)
            for k in S3_SCALARS + [rnd.randrange(1 << 64)]:
                e = es[(n + k) % len(es)]
                out.append((op, F, (pt, k), proj_line(F, X, Y, Z, (0, 0, 0), e) + [k]))
    for pt in points["g2"]:
        out.append(("X2", _Fp2, (pt,), limbs_of(_Fp2, pt[0]) + limbs_of(_Fp2, pt[1])))
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dblcheck_" + request.param) / "dblcheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_fp2_lanes_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + ["-I", CSRC, SRC, "-o", out])
    return out


def test_doubling_steps_and_chains(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(op + " " + " ".join(str(v) for v in line) + "\n" for op, _, _, line in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, f"dblcheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    seen = set()
    for i, ((op, F, val, _), line) in enumerate(zip(items, lines)):
        w = [int(x) for x in line.split()]
        seen.add(op)
        if op in ("D1", "D2"):
            X, Y, Z = val
            new, ref = [take(F, w, j) for j in range(3)], [take(F, w, j) for j in range(3, 6)]
            assert new == ref, (i, op)  # the same field elements
            assert tuple(new) == alg9(F, X, Y, Z)[:3], (i, op)
            E = E1 if F is _Fp else E2
            A = to_affine(F, X, Y, Z)
            if A is None or E.on_curve(A):
                assert to_affine(F, *new) == E.dbl(A), (i, op)
        elif op == "L2":
            X, Y, Z, px, py = val
            new, ref = [take(F, w, j) for j in range(6)], [take(F, w, j) for j in range(6, 12)]
            assert new == ref, i
            X3, Y3, Z3, t1, t2 = alg9(F, X, Y, Z)
            l01 = small(F, 3 * px, F.sqr(X))
            l11 = F.neg(small(F, 2 * py, t1))
            assert tuple(new) == (F.sub(t2, F.sqr(Y)), l01, l11, X3, Y3, Z3), i
        elif op in ("S1", "S2"):
            pt, k = val
            E = E1 if F is _Fp else E2
            new, ref = [take(F, w, j) for j in range(3)], [take(F, w, j) for j in range(3, 6)]
            exp = E.mul(pt, k)
            assert to_affine(F, *new) == exp, (i, op, hex(k))
            assert to_affine(F, *ref) == exp, (i, op, hex(k))
        else:
            (pt,) = val
            mixed, full = [take(F, w, j) for j in range(3)], [take(F, w, j) for j in range(3, 6)]
            assert mixed == full, i  # algorithm 8 gives algorithm 7's values at Z = 1
            assert to_affine(F, *mixed) == E2.mul(pt, X_ABS), i
            assert w[-2:] == [int(in_g2_psi(pt))] * 2, i
    assert seen == {"D1", "D2", "L2", "S1", "S2", "X2"}
