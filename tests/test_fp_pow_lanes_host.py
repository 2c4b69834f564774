"""The one-element-per-lane squaring pass and fixed-exponent power of lodestar_amd/csrc/
lsg_fp2_lanes.hpp (lanes_sqr_pass, lanes_pow_plan: what a gfx950 lane of k_fp_pow_lanes runs) on
the CPU, through the stand-alone driver tests/native/powlanecheck.cpp.  Built once plainly and
once with UBSan -- a column of the 64-bit accumulators that overflowed would trap -- and run
directly.  The driver itself compares, word for word, the squaring pass with the product pass
on (a, a) and the lane-form power with the one-lane host build of the pair form's
pair_pow_plan for all three plan ids; what it prints is compared here with Python integers and
pow(x, e, p) of the oracle's field.  Exact comparisons only; a failed compile is an error."""
import os
import random
import shutil
import subprocess

import pytest

from oracle.fields import P as ORACLE_P
from tests import field_edges as fe
from tests import sqr_patterns as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "powlanecheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}
P, RINV, R = sp.P, sp.RINV, 1 << 406
EXPONENTS = (P - 2, (P + 1) // 4, (P - 3) // 4)  # plan ids 0, 1, 2
HI, LO = (1 << 29) + 8, -8


def _non_residues(r, n):
    out = []
    while len(out) < n:
        x = r.randrange(2, P)
        if pow(x, (P - 1) // 2, P) == P - 1:
            out.append(x)
    return out


@pytest.fixture(scope="module")
def items():
    """limb vectors of Montgomery-form elements"""
    assert ORACLE_P == P
    r = random.Random(1711)
    out = []
    # 0, 1, p - 1 and non-residues, in Montgomery form, in every lazy representation
    for x in [0, 1, P - 1, 2, P - 2] + _non_residues(r, 6):
        out += [fe.rep(x * R % P, e) for e in fe.E_VECTORS.values()]
    # the edge values (multiples of p, +-1, the halves) in a lazy representation each
    es = list(fe.E_VECTORS.values())
    out += [fe.rep(v, es[k % len(es)]) for k, (v, _) in enumerate(fe.canon_values())]
    # the lazy bounds: every limb at one end of the carried range, the top limb at both ends
    out += [sp.clamp([lo] * 13 + [top]) for lo in (HI, LO) for top in (sp.TOP_MAX, -sp.TOP_MAX)]
    out += sp.fp_items()[:40]
    out += [sp.clamp([r.randrange(LO, HI + 1) for _ in range(13)] + [r.randrange(-sp.TOP_MAX, sp.TOP_MAX + 1)])
            for _ in range(60)]
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("powlanecheck_" + request.param) / "powlanecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_fp2_lanes_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + ["-I", CSRC, SRC, "-o", out])
    return out


def test_square_and_powers_against_the_pair_form_integers_and_the_oracle(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(" ".join(str(v) for v in it) + "\n" for it in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    # status 1: the driver found the lane form and the pair form (or the two passes) to differ
    assert p.returncode == 0 and not p.stderr, f"powlanecheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    for i, (it, line) in enumerate(zip(items, lines)):
        w = [int(x) for x in line.split()]
        assert len(w) == 56
        sq, pw = w[:14], [w[14 * k:14 * k + 14] for k in range(1, 4)]
        a = sp.value(it)
        x = a * RINV % P  # the field element the limbs stand for
        assert (sp.value(sq) - a * a * RINV) % P == 0, i
        assert sp.value(sq) * RINV % P == x * x % P, i
        for e, r in zip(EXPONENTS, pw):
            assert sp.value(r) * RINV % P == pow(x, e, P), (i, e)
            assert abs(sp.value(r)) < 3 * P, (i, e)
        assert all(0 <= v < (1 << 29) for e in [sq] + pw for v in e[:13]), i
