"""The variable-size LSG_MSG_OBJECT kinds on the CPU: ssz_var_step of
lodestar_amd/csrc/lsg_ssz.hpp (the text k_msg_roots_var runs, one 64-lane workgroup per object)
stepped over 64 logical lanes by tests/native/sszvarcheck.cpp, altair.ContributionAndProof, the
zero-subtree table, and the host policy of lodestar_amd/csrc/lsg_plan.hpp (the three fields of
a marked length word, the structural check).  The driver is built with AddressSanitizer and
UBSan, as tests/test_ssz_roots_host.py builds its own.  Expected roots: tests/msgobjects_var.py
(unpinned beyond the SSZ spec).  Exact comparisons only."""
import hashlib
import os
import random
import shutil
import subprocess

import pytest

from tests import msgobjects_var as mv

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sszvarcheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MARK = 0x80000000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sszvarcheck") / "sszvarcheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", out])
    return out


def run(exe, *args):
    p = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, f"sszvarcheck exit {p.returncode}: {p.stderr[-2000:]}"
    return p.stdout


def roots(exe, tmp_path, cases):
    """cases: [(kind, object, domain)] -> [[root, root over the payload, dependent, bound]]"""
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(f"{k} {o.hex()} {d.hex()}\n" for k, o, d in cases))
    run(exe, "roots", src, out)
    lines = [ln.split() for ln in open(out).read().split("\n")[:-1]]
    assert len(lines) == len(cases)
    return lines


def bound(kind, n_bits):
    """sum over the levels of the chunk tree of ceil(pairs / 64), plus 15 for the containers
    (AttestationData 9, length mix-in 1, Attestation 2, AggregateAndProof 2, SigningData 1)"""
    cnt, total = max((n_bits + 255) // 256, 1), 0
    for _ in range(9 if kind == mv.AGG_PROOF_ELECTRA else 3):
        pairs = (cnt + 1) // 2
        total += (pairs + 63) // 64
        cnt = pairs
    return total + 15


@pytest.mark.parametrize("kind", [mv.AGG_PROOF, mv.AGG_PROOF_ELECTRA])
def test_roots_and_dependent_counts(exe, tmp_path, kind):
    cs = mv.cases(kind)
    assert len(cs) == 3 * len(mv.BIT_COUNTS[kind])
    got = roots(exe, tmp_path, [(kind, c[2], c[3]) for c in cs])
    for (n, fill, obj, dom, want, _), (own, over, dep, bnd) in zip(cs, got):
        assert own == over == want.hex(), (kind, n, fill)  # its own buffer; over the payload
        # the structural condition: depth + chunks / 128, not the chunk count
        assert int(bnd) == bound(kind, n) and 0 < int(dep) <= bound(kind, n), (kind, n, dep, bnd)
    assert bound(mv.AGG_PROOF_ELECTRA, 131072) == 28 and bound(mv.AGG_PROOF_ELECTRA, 28800) == 24 and bound(mv.AGG_PROOF, 2048) == 18


def test_contribution_and_proof(exe, tmp_path):
    rng = random.Random(264)
    cases = [(bytes(264), bytes(32)), (b"\xff" * 264, b"\xff" * 32)] + [(rng.randbytes(264), rng.randbytes(32)) for _ in range(50)]
    got = roots(exe, tmp_path, [(0, o, d) for o, d in cases])
    for (o, d), (own, over, _, _) in zip(cases, got):
        assert own == over == mv.signing_root(mv.contribution_and_proof_root(o), d).hex()


def test_zero_hash_table(exe):
    want, z = [], bytes(32)
    for _ in range(10):
        want.append(z.hex())
        z = hashlib.sha256(z + z).digest()
    assert run(exe, "zero").split() == want


def test_classification_of_every_tag(exe):
    rows = [[int(x) for x in ln.split()] for ln in run(exe, "classify").splitlines()]
    lens = [0, 32, 160, 296, 369, 0x00ffffff]
    assert [(r[0], r[1]) for r in rows] == [(t, n) for t in range(128) for n in lens]
    fixed = {160: 128, 296: 264}
    for tag, n, m_bytes, m_tag, m_marked, m_fixed, m_kind, u_bytes, u_tag, u_marked, u_fixed, u_kind in rows:
        # marked: marker, tag, payload length
        assert (m_bytes, m_tag, m_marked, m_fixed) == (n, tag, 1, int(tag == 0))
        assert m_kind == (fixed.get(n, 0) if tag == 0 else 0)  # the length selects a kind under tag 0 only
        # unmarked: a byte count in all its bits (2^24 and above included), no tag, no kind
        assert (u_bytes, u_tag, u_marked, u_fixed, u_kind) == ((tag << 24) | n, 0, 0, 0, 0)


def test_argument_check(exe):
    assert run(exe, "args") == "ok\n"
