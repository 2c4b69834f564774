"""The squaring leaves of lodestar_amd/csrc/lsg_fp_pair.hpp on the CPU, in the one-lane build
(LSG_PAIR_G = 1), through the stand-alone driver tests/native/sqrcheck.cpp: built once plainly
and once with UBSan (signed-integer overflow in the 64-bit accumulators is the bound the leaves
argue), and run directly.  The driver compares pair_mont_sqr(a) with pair_mont_mul(a, a) limb
for limb; the values are compared here with Python integers, at the lazy bounds of the inputs
(tests/sqr_patterns.py).  Exact comparisons only."""
import os
import shutil
import subprocess

import pytest

from tests import sqr_patterns as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sqrcheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module")
def items():
    fp = sp.fp_items()
    f2 = sp.fp2_items()
    assert len(fp) == len(f2)
    # a0 of item k is the k-th Fp pattern (mixes included), a1 the Fp2 walk's partner
    return [(fp[k], f2[k][1]) for k in range(len(fp))] + f2


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sqrcheck_" + request.param) / "sqrcheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + ["-I", CSRC, SRC, "-o", out])
    return out


def test_squaring_leaves_against_integers(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(" ".join(str(v) for v in a0 + a1) + "\n" for a0, a1 in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, f"sqrcheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    for i, ((a0, a1), line) in enumerate(zip(items, lines)):
        w = [int(x) for x in line.split()]
        assert len(w) == 42
        s, c0, c1 = w[:14], w[14:28], w[28:]
        v0, v1 = sp.value(a0), sp.value(a1)
        assert (sp.value(s) - v0 * v0 * sp.RINV) % sp.P == 0, i
        assert (sp.value(c0) - (v0 * v0 - v1 * v1) * sp.RINV) % sp.P == 0, i
        assert (sp.value(c1) - 2 * v0 * v1 * sp.RINV) % sp.P == 0, i
        assert abs(sp.value(s)) < 2 * sp.P and abs(sp.value(c0)) < 3 * sp.P and abs(sp.value(c1)) < 3 * sp.P, i
        assert all(0 <= x < (1 << 29) for x in s[:13] + c0[:13] + c1[:13]), i
