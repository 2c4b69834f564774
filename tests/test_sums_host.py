"""The lazy sums of lodestar_amd/csrc/lsg_fp_pair.hpp and every formula rewritten with them, on the
CPU in the one-lane build (LSG_PAIR_G = 1), through the stand-alone driver tests/native/sumcheck.cpp.
The driver is built four times and run directly, never loaded into Python:
  lazy    the shipped form: uncarried sums, one carry round per group
  eager   -DLSG_EAGER_SUMS: every operation carried, the formulas as they were
  ubsan   the lazy form with UBSan (32-bit wrap of a signed limb is the bound the types argue)
  audit   -DLSG_SUM_AUDIT: every lazy limb shadowed in 64 bits; aborts when a limb at a carry is
          outside the range its type promises or a product operand outside the carried range
Every output integer (sum of limb 2^(29 k), not reduced mod p) of the lazy, ubsan and audit builds
must equal the eager build's; the sums and small multiples, which involve no product, are also
compared with Python integers.  The driver itself compares the fused Miller kernel's regrouped
combinations with the nested forms they replaced.  Inputs: the limb patterns of
tests/sqr_patterns.py plus the closed upper end 2^29 + 8 of a carried limb."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import sqr_patterns as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sumcheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"lazy": ["-O2"],
          "eager": ["-O2", "-DLSG_EAGER_SUMS"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"],
          "audit": ["-O2", "-DLSG_SUM_AUDIT"]}
LIMB_MIN, LIMB_MAX = -8, (1 << 29) + 8
HEAVY = 6  # items that also run the chains (sumcheck.cpp)


@pytest.fixture(scope="module")
def items():
    top = [clamped for clamped in (sp.clamp([LIMB_MAX] * 13 + [1]), sp.clamp([LIMB_MAX] * 13 + [-1]))]
    return sp.fp2_items() + [(top[0], top[1]), (top[1], top[0])]


@pytest.fixture(scope="module")
def outputs(items, tmp_path_factory):
    """{build: per item the list of output integers}"""
    d = tmp_path_factory.mktemp("sumcheck")
    gxx = shutil.which("g++")
    if gxx:
        cc = [gxx, "-std=c++17"]
    else:  # as tests/test_sqr_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cc = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    src = str(d / "in.txt")
    with open(src, "w") as fh:
        fh.write("".join(" ".join(str(v) for v in a0 + a1) + "\n" for a0, a1 in items))

    def one(name):
        exe, dst = str(d / ("sumcheck_" + name)), str(d / (name + ".txt"))
        subprocess.check_call(cc + BUILDS[name] + ["-I", CSRC, SRC, "-o", exe])
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, f"sumcheck[{name}] exit {p.returncode}: {p.stderr[-2000:]}"
        assert p.stdout.split() == [str(len(items))]
        rows = []
        for line in open(dst).read().split("\n")[:-1]:
            w = [int(x) for x in line.split()]
            assert len(w) % 14 == 0
            rows.append([w[k:k + 14] for k in range(0, len(w), 14)])
        assert len(rows) == len(items)
        return rows

    with ThreadPoolExecutor(max_workers=len(BUILDS)) as ex:
        return dict(zip(sorted(BUILDS), ex.map(one, sorted(BUILDS))))


@pytest.mark.parametrize("build", ["lazy", "ubsan", "audit"])
def test_every_output_integer_equals_the_eager_build(outputs, build):
    ref, got = outputs["eager"], outputs[build]
    n_light = len(ref[-1])
    for i, (r, g) in enumerate(zip(ref, got)):
        assert len(r) == len(g) and len(r) == (n_light if i >= HEAVY else len(ref[0])), i
        assert len(ref[0]) > n_light
        for k, (x, y) in enumerate(zip(r, g)):
            assert sp.value(x) == sp.value(y), (i, k)


@pytest.mark.parametrize("build", ["lazy", "eager"])
def test_sums_and_small_multiples_against_integers(outputs, items, build):
    ring = [e for it in items for e in it]
    n = len(ring)
    for i, row in enumerate(outputs[build]):
        a, b, c, d, e, f = (sp.value(ring[(2 * i + j) % n]) for j in range(6))
        want = [a + b + c - d - e - f, 2 * a, 3 * a, 4 * a, 8 * a, 12 * a, 2 * (a + b + c - d - e - f),
                4 * (a + b + c - d), 8 * (a + b), -a - b - c + d]
        for k, w in enumerate(want):
            assert sp.value(row[k]) == w, (i, k)
            if build == "lazy":  # what carry() and carry_mul() promise: a carried limb vector
                assert all(LIMB_MIN <= x <= LIMB_MAX for x in row[k][:13]), (i, k, row[k])
        # fp2_mul_xi, fp2_mul_b3 = 12 (1 + u) a and fp_mul12 (outputs 10..14)
        x0, x1 = a, b
        assert [sp.value(v) for v in row[10:15]] == [x0 - x1, x0 + x1, 12 * (x0 - x1), 12 * (x0 + x1), 12 * a], i
