"""The two per-lane operations the fused Miller kernel adds to lodestar_amd/csrc/lsg_fp2_lanes.hpp
-- the Fp2 x Fp product (one pass per lane, the Fp factor on both lanes) and the product by
xi = 1 + u as a lazy sum -- on the CPU, through the stand-alone driver
tests/native/mflanecheck.cpp: the code a gfx950 lane runs, with its partner lane simulated by the
driver.  Built once plainly and once with UBSan -- a column of the 64-bit accumulators that
overflowed would trap -- and run directly.  The outputs are compared with Python integers and with
the oracle's Fp2 arithmetic (oracle/fields.py) on the edge values of tests/field_edges.py in every
lazy representation, the limb extremes of tests/sqr_patterns.py and random values.  Exact
comparisons only; a failed compile is an error."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

from oracle.fields import f2_mul
from tests import field_edges as fe
from tests import sqr_patterns as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "mflanecheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}
P, RINV = sp.P, sp.RINV
HI, LO = (1 << 29) + 8, -8


@pytest.fixture(scope="module")
def items():
    """(a0, a1, k) limb vectors"""
    out = []
    # the edge values (multiples of p, +-1, the halves) in every lazy representation
    reps = [fe.rep(v, e) for v, _ in fe.canon_values() for e in fe.E_VECTORS.values()]
    n = len(reps)
    out += [(reps[k], reps[(3 * k + 1) % n], reps[(5 * k + 2) % n]) for k in range(n)]
    # every limb at one end of the carried range, the top limb at both ends of its range
    ext = [[lo] * 13 + [top] for lo, top in itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX, HI, LO))]
    out += [(a0, a1, k) for a0, a1, k in itertools.product(ext, ext, ext)]
    f2 = sp.fp2_items()
    out += [f2[k] + (f2[(7 * k + 3) % len(f2)][k % 2],) for k in range(len(f2))]
    r = random.Random(1511)

    def rnd():
        return sp.clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)])
    out += [(rnd(), rnd(), rnd()) for _ in range(200)]
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mflanecheck_" + request.param) / "mflanecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_fp2_lanes_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + ["-I", CSRC, SRC, "-o", out])
    return out


def test_mul_fp_and_xi_against_integers_and_the_oracle(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(" ".join(str(v) for e in it for v in e) + "\n" for it in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, f"mflanecheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    for i, (it, line) in enumerate(zip(items, lines)):
        w = [int(x) for x in line.split()]
        assert len(w) == 56
        m0, m1, x0, x1 = (w[14 * k:14 * k + 14] for k in range(4))
        a0, a1, k = (sp.value(e) for e in it)
        # each lane: (a_c k) / R mod p
        assert (sp.value(m0) - a0 * k * RINV) % P == 0, i
        assert (sp.value(m1) - a1 * k * RINV) % P == 0, i
        # the oracle's field: the Montgomery form of its product with (k, 0)
        A, K = (a0 * RINV % P, a1 * RINV % P), (k * RINV % P, 0)
        assert tuple(sp.value(x) * RINV % P for x in (m0, m1)) == f2_mul(A, K), i
        assert all(0 <= x < (1 << 29) for e in (m0, m1) for x in e[:13]), i
        # xi a = (c0 - c1) + (c0 + c1) u: the integers, exactly, limb by limb
        assert x0 == [p0 - p1 for p0, p1 in zip(it[0], it[1])], i
        assert x1 == [p1 + p0 for p0, p1 in zip(it[0], it[1])], i
        assert (sp.value(x0), sp.value(x1)) == (a0 - a1, a0 + a1), i
