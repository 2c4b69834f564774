"""The SSZ signing roots of LSG_MSG_OBJECT sets on the CPU: the functions of
lodestar_amd/csrc/lsg_ssz.hpp that k_msg_roots and the signing-root kernels run on the device,
and the host policy of lodestar_amd/csrc/lsg_plan.hpp (payload length -> kind, the argument
check), through the stand-alone driver tests/native/sszcheck.cpp built with AddressSanitizer
and UBSan.  Every root is compared with oracle/interop.py's helpers (tests/msgobjects.py).
Exact comparisons only."""
import os
import random
import shutil
import subprocess

import pytest

from tests import msgobjects as mo

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sszcheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MARK = 0x80000000
PAYLOAD_KIND = {40: 8, 48: 16, 64: 32, 108: 76, 120: 88, 144: 112, 160: 128}  # the issue's table


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sszcheck") / "sszcheck")
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
    assert p.returncode == 0 and not p.stderr, f"sszcheck exit {p.returncode}: {p.stderr[-2000:]}"
    return p.stdout


def test_roots_of_every_kind_match_the_oracle(exe, tmp_path):
    rng = random.Random(86)
    cases = []
    for n in mo.KINDS:
        cases.append((bytes(n), bytes(32)))
        cases.append((b"\xff" * n, b"\xff" * 32))
        cases += [(rng.randbytes(n), rng.randbytes(32)) for _ in range(50)]
    kat_obj, kat_dom, kat_root = mo.genesis_kat()
    cases.append((kat_obj, kat_dom))
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(f"{o.hex()} {d.hex()}\n" for o, d in cases))
    run(exe, "roots", src, out)
    lines = open(out).read().split("\n")[:-1]
    assert len(lines) == len(cases) == 7 * 52 + 1
    for (o, d), line in zip(cases, lines):
        want = mo.signing_root(o, d).hex()
        assert line.split() == [want, want], (len(o), o.hex(), d.hex())  # its own buffer; over the payload
    assert lines[-1].split()[0] == kat_root.hex()


def test_lengths_that_name_no_kind_store_nothing(exe, tmp_path):
    rng = random.Random(5)
    lens = [n for n in range(0, 201) if n not in mo.KINDS]
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(f"{rng.randbytes(n).hex() or '-'} {rng.randbytes(32).hex()}\n" for n in lens))
    run(exe, "roots", src, out)
    assert open(out).read() == "- -\n" * len(lens)


def test_classification_of_every_length(exe):
    rows = [[int(x) for x in line.split()] for line in run(exe, "classify").splitlines()]
    assert [r[0] for r in rows] == list(range(201))
    for length, unmarked, marked, nbytes, is_marked in rows:
        assert unmarked == 0 and is_marked == 0  # an unmarked length names no kind, whatever it is
        assert marked == PAYLOAD_KIND.get(length, 0), length
        assert nbytes == length  # the marker is not part of the byte count
    assert sorted(k + 32 for k in mo.KINDS) == sorted(PAYLOAD_KIND)


def test_argument_check(exe):
    assert run(exe, "args") == "ok\n"
