"""The per-lane passes of lodestar_amd/csrc/lsg_fp2_lanes.hpp (the Fp2 layout with one component
per lane) on the CPU, through the stand-alone driver tests/native/fp2lanecheck.cpp: the code a
gfx950 lane runs, with its partner lane simulated by the driver.  Built once plainly and once with
UBSan -- a column of the 64-bit accumulators that overflowed would trap -- and run directly.  The
outputs are compared with Python integers and with the oracle's Fp2 arithmetic (oracle/fields.py)
on the edge values of tests/field_edges.py in every lazy representation, the limb extremes of
tests/sqr_patterns.py and random values.  Exact comparisons only; a failed compile is an error."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

from oracle.fields import f2_mul, f2_sqr
from tests import field_edges as fe
from tests import sqr_patterns as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fp2lanecheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}
P, RINV = sp.P, sp.RINV
HI, LO = (1 << 29) + 8, -8


@pytest.fixture(scope="module")
def items():
    """(a0, a1, b0, b1) limb vectors"""
    out = []
    # the edge values (multiples of p, +-1, the halves) in every lazy representation
    reps = [fe.rep(v, e) for v, _ in fe.canon_values() for e in fe.E_VECTORS.values()]
    n = len(reps)
    out += [(reps[k], reps[(3 * k + 1) % n], reps[(5 * k + 2) % n], reps[(7 * k + 3) % n]) for k in range(n)]
    # every limb at one end of the carried range, the top limb at both ends of its range
    ext = [[lo] * 13 + [top] for lo, top in itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX, HI, LO))]
    out += [(a0, a1, a0, a1) for a0, a1 in itertools.product(ext, ext)]
    out += [(a0, a1, a1, a0) for a0, a1 in itertools.product(ext, ext)]
    f2 = sp.fp2_items()
    out += [f2[k] + f2[(7 * k + 3) % len(f2)] for k in range(len(f2))]
    r = random.Random(1409)

    def rnd():
        return sp.clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)])
    out += [(rnd(), rnd(), rnd(), rnd()) for _ in range(200)]
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fp2lanecheck_" + request.param) / "fp2lanecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_sqr_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + ["-I", CSRC, SRC, "-o", out])
    return out


def test_lane_passes_against_integers_and_the_oracle(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(" ".join(str(v) for e in it for v in e) + "\n" for it in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, f"fp2lanecheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    for i, (it, line) in enumerate(zip(items, lines)):
        w = [int(x) for x in line.split()]
        assert len(w) == 56
        m0, m1, s0, s1 = (w[14 * k:14 * k + 14] for k in range(4))
        a0, a1, b0, b1 = (sp.value(e) for e in it)
        assert (sp.value(m0) - (a0 * b0 - a1 * b1) * RINV) % P == 0, i
        assert (sp.value(m1) - (a0 * b1 + a1 * b0) * RINV) % P == 0, i
        assert (sp.value(s0) - (a0 * a0 - a1 * a1) * RINV) % P == 0, i
        assert (sp.value(s1) - 2 * a0 * a1 * RINV) % P == 0, i
        # the oracle's field: the Montgomery forms of its product and square
        A, B = (a0 * RINV % P, a1 * RINV % P), (b0 * RINV % P, b1 * RINV % P)
        assert tuple(sp.value(x) * RINV % P for x in (m0, m1)) == f2_mul(A, B), i
        assert tuple(sp.value(x) * RINV % P for x in (s0, s1)) == f2_sqr(A), i
        if all(abs(sp.value(e)) < sp.BOUND for e in it):  # operands inside a lazy value's bound, 2^12.6 p
            assert all(abs(sp.value(x)) < 3 * P for x in (m0, m1, s0, s1)), i
        assert all(0 <= x < (1 << 29) for e in (m0, m1, s0, s1) for x in e[:13]), i
