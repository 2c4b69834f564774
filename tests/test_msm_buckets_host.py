"""The bucket pass of the signature MSM on the CPU: its plan and its fold.

a) plan_buckets (lodestar_amd/csrc/lsg_plan.hpp), reached through plan_phase as the host reaches
   it, by the stand-alone driver tests/native/bucketplancheck.cpp built with AddressSanitizer and
   UBSan: the new plan and the one it replaces (plan_seg's) replayed on integers against direct
   sums for 256, 257, 4,096 and 32,768 sets with random randomizers, all-equal randomizers (eight
   full buckets, a second pass), randomizers with zero digits and two groups of different window
   widths; the limits of a chunk; a small group stays at one lane pair per bucket; for 32,768 sets
   the modelled lane-pair additions are at most 0.65 of the present plan's (both counted by the
   driver from the two plans).
b) g2_fold_mixed (lsg_curve.hpp), the arithmetic of k_msm_bucket_seg, by
   tests/native/bucketfoldcheck.cpp on the one-lane host build of the pair backend, plain and
   under UBSan: first member, mixed additions, the skip rule and the butterfly order against the
   plain sum and the oracle's group law.  Exact comparisons only; a failed compile is an error."""
import os
import random
import shutil
import subprocess

import pytest

from oracle.curves import E2, G2_GEN, _Fp2
from oracle.fields import P
from tests import field_edges as fe

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}


def compiler():
    gxx = shutil.which("g++")
    if gxx:
        return [gxx, "-std=c++17"]
    from lodestar_amd.build import hipcc  # the build's own compiler, host side only
    return [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]


# ---------------------------------------------------------------- a) the plan
@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("bucketplancheck")
    exe, out = str(d / "bucketplancheck"), str(d / "out.txt")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(compiler() + flags + [os.path.join(HERE, "native", "bucketplancheck.cpp"), "-o", exe])
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, f"bucketplancheck exit {p.returncode}: {p.stderr[-2000:]}"
    rows = {}
    for line in open(out).read().splitlines():
        w = line.split()
        rows[w[0]] = dict(sets=int(w[2]), groups=int(w[4]), ips=int(w[6]), passes=int(w[8]), waves=int(w[10]),
                          adds=int(w[12]), chain=int(w[14]), old_ips=int(w[16]), old_passes=int(w[18]), old_adds=int(w[20]))
    assert p.stdout.split() == [str(len(rows))]
    return rows


def test_bucket_plan_cases_ran(plan_lines):
    assert sorted(plan_lines) == sorted(["random256", "random257", "random4096", "random32768", "equal4096",
                                         "zerodigits4096", "widths2048+255"])
    for name, r in plan_lines.items():
        assert 0 <= r["ips"] <= 5 and r["passes"] <= r["old_passes"], name
        if name in ("random256", "random257"):  # no bucket past SEG_FOLD members: plan_seg's plan, word for word
            assert (r["ips"], r["passes"], r["adds"]) == (r["old_ips"], r["old_passes"], r["old_adds"]), name
        else:
            assert r["adds"] < r["old_adds"], name  # the order alone saves where the pairs stay
    for name in ("random4096", "random32768", "equal4096"):
        assert plan_lines[name]["ips"] < plan_lines[name]["old_ips"], name  # fewer pairs than plan_seg takes


def test_small_groups_stay_at_one_pair(plan_lines):
    for name in ("random256", "random257"):
        assert plan_lines[name]["ips"] == 0 and plan_lines[name]["old_ips"] == 0 and plan_lines[name]["passes"] == 1


def test_full_buckets_take_a_second_pass(plan_lines):
    assert plan_lines["equal4096"]["passes"] == 2 and plan_lines["equal4096"]["old_passes"] == 2


def test_firehose_plan_is_work_bound(plan_lines):
    r = plan_lines["random32768"]
    print("32,768 sets: ips_log2 %d, %d waves, %d lane-pair additions (present plan: ips_log2 %d, %d), chain %d"
          % (r["ips"], r["waves"], r["adds"], r["old_ips"], r["old_adds"], r["chain"]))
    assert r["old_ips"] == 5 and r["passes"] == 1
    assert r["adds"] <= 0.65 * r["old_adds"]


# ---------------------------------------------------------------- b) the fold
def mont(v):
    return fe.rep(v * fe.R % P, fe.E_VECTORS["zero"])


def canon(limbs):
    return fe.value(limbs) * fe.RINV % P


def take2(w, i):
    c = w[28 * i:28 * i + 28]
    return (canon(c[:14]), canon(c[14:]))


def to_affine(X, Y, Z):
    if _Fp2.is_zero(Z):
        return None
    zi = _Fp2.inv(Z)
    return (_Fp2.mul(X, zi), _Fp2.mul(Y, zi))


@pytest.fixture(scope="module")
def chunks():
    """[(ips_log2, [(use, point)])]: every length around the lane pairs of a chunk, the same point
    twice (a doubling inside the mixed addition), P then -P then more (the sum returns to the
    identity mid-fold), nobody taking part, a skipped member first and last"""
    rnd = random.Random(414)
    pts = [E2.mul(G2_GEN, rnd.randrange(1, R_ORDER)) for _ in range(12)]

    def pick(n):
        return [(1, pts[rnd.randrange(len(pts))]) for _ in range(n)]

    out = []
    for l in (0, 1, 2, 3, 5):
        ips = 1 << l
        for n in sorted({0, 1, ips - 1, ips, ips + 1, 2 * ips + 1, 3 * ips}):
            if n >= 0:
                out.append((l, pick(n)))
    A, B = pts[0], pts[1]
    for l in (0, 1, 2):
        ips = 1 << l
        # lane pair 0 meets members 0, ips, 2 ips, ...: the special sequences sit at that stride
        def strided(seq, ips=ips):
            m = pick(ips * len(seq))
            for k, v in enumerate(seq):
                m[ips * k] = v
            return m
        out.append((l, strided([(1, A), (1, A), (1, B)])))                      # doubling
        out.append((l, strided([(1, A), (1, A), (1, A)])))                      # ... and 2A + A
        out.append((l, strided([(1, A), (1, E2.neg(A)), (1, B), (1, B)])))      # back to the identity, then on
        out.append((l, strided([(1, A), (1, E2.neg(A))])))                      # ends at the identity
        out.append((l, strided([(0, A), (1, B), (1, A), (0, B)])))              # skipped first and last
        out.append((l, [(0, p) for _, p in pick(2 * ips + 1)]))                  # nobody takes part
    out.append((2, [(1, A), (1, A), (1, A), (1, A), (1, A)]))                   # equal partial sums in the butterfly
    out.append((1, [(1, A), (1, E2.neg(A))]))                                   # opposite partial sums
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def fold_exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bucketfoldcheck_" + request.param) / "bucketfoldcheck")
    src = os.path.join(HERE, "native", "bucketfoldcheck.cpp")
    subprocess.check_call(compiler() + BUILDS[request.param] + ["-I", CSRC, src, "-o", out])
    return out


def test_fold_against_plain_sum_and_oracle(fold_exe, chunks, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        for l, members in chunks:
            fh.write("C %d %d\n" % (l, len(members)))
            for use, (x, y) in members:
                fh.write("%d %s\n" % (use, " ".join(str(v) for v in mont(x[0]) + mont(x[1]) + mont(y[0]) + mont(y[1]))))
    p = subprocess.run([fold_exe, src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, f"bucketfoldcheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(chunks))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(chunks)
    met_identity = 0
    for i, ((l, members), line) in enumerate(zip(chunks, lines)):
        w = [int(v) for v in line.split()]
        fold = to_affine(*[take2(w, j) for j in range(3)])
        plain = to_affine(*[take2(w, j) for j in range(3, 6)])
        want = None
        for use, pt in members:
            if use:
                want = E2.add(want, pt)
        assert fold == want, (i, l, len(members))
        assert plain == want, (i, l, len(members))
        met_identity += want is None
    assert met_identity >= 8
