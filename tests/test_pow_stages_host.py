"""The stages that the signature decode and the SSWU map are cut into around their two powers
(fp2_sqrt_root_c / fp2_sqrt_root_finish, g2_uncompress_parse / g2_uncompress_finish,
sswu_stage_a / b / c), composed as the stage kernels compose them with each power run by the
one-element-per-lane lanes_pow_plan, against the unsplit functions: the stand-alone driver
tests/native/powstagecheck.cpp (one-lane host build of the pair backend) compares the two limb
for limb and exits with status 1 at a difference; what it prints is compared here with the
oracle.  Built once plainly and once with UBSan, run directly.  A failed compile is an error."""
import json
import os
import random
import subprocess

import pytest

from oracle import hash_to_curve as h2c
from oracle.curves import BlstError, g2_serialize, g2_uncompress
from oracle.fields import P

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "powstagecheck.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {"plain": ["-O2"],
          "ubsan": ["-O1", "-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=undefined"]}


def be(v):
    return int(v).to_bytes(48, "big")


@pytest.fixture(scope="module")
def items():
    """[(kind, 96 bytes)]: signatures (valid, not on the curve, flag and range errors, infinity,
    x = 0) and field elements u (0, the exceptional tv1 = 0 values, +-1, random)"""
    r = random.Random(1712)
    out = [("S", bytes.fromhex(h)) for h in json.load(open(os.path.join(HERE, "golden", "mainnet_g2_points.json")))[:12]]
    out += [("S", bytes.fromhex(it["sig"])) for it in json.load(open(os.path.join(HERE, "golden", "mainnet_g2_points_bad.json")))[:6]]
    for _ in range(24):  # random x: on the curve about half the time
        b = bytearray(be(r.randrange(P)) + be(r.randrange(P)))
        b[0] |= 0x80 | (0x20 if r.random() < 0.5 else 0)
        out.append(("S", bytes(b)))
    out.append(("S", bytes([0xC0]) + bytes(95)))            # infinity
    out.append(("S", bytes([0xC0]) + bytes(94) + b"\x01"))  # infinity flag with a set bit
    out.append(("S", bytes(96)))                             # no compression flag
    out.append(("S", bytes([0x80]) + bytes(95)))            # x = 0
    out.append(("S", bytes([0x80 | 0x1A]) + b"\xff" * 95))  # x1 >= p
    out.append(("S", bytes([0x80]) + bytes(47) + be(P)))     # x0 = p
    us = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1)]
    us += [(r.randrange(P), r.randrange(P)) for _ in range(24)]
    for u in us:
        out += [("M", be(u[0]) + be(u[1])), ("M", be(-u[0] % P) + be(-u[1] % P))]
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    from lodestar_amd.build import hipcc
    out = str(tmp_path_factory.mktemp("powstagecheck_" + request.param) / "powstagecheck")
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"] + BUILDS[request.param] +
                          ["-I", CSRC, SRC, "-o", out])
    return out


def test_staged_decode_and_map_equal_the_unsplit_functions_and_the_oracle(exe, items, tmp_path):
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(src, "w") as fh:
        fh.write("".join(f"{k} {b.hex()}\n" for k, b in items))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, f"powstagecheck exit {p.returncode}: {p.stderr[-2000:]}"
    assert p.stdout.split() == [str(len(items))]
    lines = open(dst).read().split("\n")[:-1]
    assert len(lines) == len(items)
    codes = set()
    for i, ((kind, b), line) in enumerate(zip(items, lines)):
        w = line.split()
        if kind == "S":
            e, inf, pt = int(w[0]), int(w[1]), bytes.fromhex(w[2])
            codes.add(e)
            try:
                exp = g2_uncompress(b)
                assert e == 0 and inf == (exp is None) and pt == g2_serialize(exp), i
            except BlstError as err:
                assert e == err.code, i
        else:
            u = (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))
            assert bytes.fromhex(w[0]) == g2_serialize(h2c.map_to_curve_sswu(u)), i
    assert {0, 1, 2} <= codes
