"""The references of tests/test_gpu_msg_lengths.py, pinned on the CPU before the device is compared
with them, over the message and DST lengths of tests/msglens.py:

- the length lists reach every tail of b_0 and of b_i at which SHA-256's padding changes shape
  (computed from the block arithmetic, not listed by hand);
- oracle.hash_to_curve.expand_message_xmd equals a restatement of RFC 9380 section 5.3.1 over
  hashlib, written here;
- three implementations of hash_to_G2 agree byte for byte: the Python oracle (at the named tails
  and the cross pairs: it takes ~25 ms a hash), the C oracle (oracle/c/bls_cpu.c) and the host
  build of the kernel headers (tests/native/hostcheck.hip: lsg_h2c.hpp's own SHA-256) at every
  case.  No GPU."""
import ctypes
import hashlib
import itertools
import subprocess

import pytest

from oracle import hash_to_curve as h2c
from oracle.curves import g2_serialize
from tests import cpu_oracle as co
from tests import msglens as ml
from tests.hostcheck_lib import build as build_hostcheck


def xmd_rfc9380(msg, dst, n=256):
    """expand_message_xmd, RFC 9380 section 5.3.1 step by step, H = SHA-256 (b = 32, s = 64)"""
    ell = -(-n // 32)                                                  # 1
    assert ell <= 255 and n <= 65535 and len(dst) <= 255               # 2
    dst_prime = dst + bytes([len(dst)])                                # 3
    z_pad = bytes(64)                                                  # 4
    l_i_b_str = n.to_bytes(2, "big")                                   # 5
    b_0 = hashlib.sha256(z_pad + msg + l_i_b_str + b"\x00" + dst_prime).digest()  # 6, 7
    b = [hashlib.sha256(b_0 + b"\x01" + dst_prime).digest()]           # 8
    for i in range(2, ell + 1):                                        # 9, 10
        x = bytes(p ^ q for p, q in zip(b_0, b[-1]))
        b.append(hashlib.sha256(x + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:n]                                             # 11, 12


def sha_blocks(n):
    """blocks SHA-256 compresses for n bytes: the data, 0x80, zeros, an 8-byte length"""
    return (n + 1 + 8 + 63) // 64


def test_pop_dst_and_32_bytes_reach_one_tail_each():
    """what the suite had: 32-byte messages under the POP DST end b_0 at 143 bytes and every
    b_i at 77, tails 15 and 13 -- neither near a change of the padding"""
    assert ml.DST_POP == h2c.DST_POP and ml.POP == 43
    assert (ml.b0_bytes(32), ml.b0_tail(32)) == (143, 15)
    assert (ml.bi_bytes(), ml.bi_tail()) == (77, 13)
    assert 15 not in ml.TAILS and 13 not in ml.TAILS


def test_named_tails_are_where_the_padding_changes():
    """the names of msglens.NAMED against the count of blocks: up to tail 55 the padding shares
    the data's last block, from 56 on it takes one more; tail 0 pads a block that holds no data"""
    for t in range(64):
        for full in (0, 1, 5):
            n = 64 * full + t
            assert sha_blocks(n) - full == (1 if t <= 55 else 2), n
    assert set(ml.NAMED) == {55, 56, 59, 60, 63, 0} and set(ml.NAMED) <= set(ml.TAILS)
    assert set(ml.TAILS) == set(range(52, 64)) | {0, 1, 2, 3}


def test_length_lists_cover_every_tail_of_both_hashes():
    small = [L for L in ml.MSG_LENS if L <= 130]
    assert small == list(range(131))
    assert set(ml.MSG_LENS) - set(small) == {191, 192, 193, 255, 256, 1000, 4099}
    assert list(ml.DST_LENS) == list(range(256))
    # b_0 under the POP DST: every tail (the named ones among them) in two cycles of L
    for t in range(64):
        assert len([L for L in small if ml.b0_tail(L) == t]) >= 2, t
    # the DST sweep: b_i's tail in four cycles, and b_0's with it
    for t in range(64):
        assert len([D for D in ml.DST_LENS if ml.bi_tail(D) == t]) == 4, t
        assert len([D for D in ml.DST_LENS if ml.b0_tail(ml.DST_MSG_LEN, D) == t]) == 4, t
    # the 16-byte chunk loop of shal_bytes: below, at and above one and two chunks, for the
    # message and for the DST; messages of several blocks; the message cache's limit
    assert {15, 16, 17, 31, 32, 33} <= set(ml.MSG_LENS) and {15, 16, 17, 31, 32, 33} <= set(ml.DST_LENS)
    assert max(ml.MSG_LENS) > 64 * 64 and {191, 192, 193} <= set(ml.MSG_LENS)
    # CROSS: every pair of b_0 and b_i tails out of 55, 56, 63 and 0, each D the ABI admits
    ends = (55, 56, 63, 0)
    assert sorted((ml.b0_tail(L, D), ml.bi_tail(D)) for L, D in ml.CROSS) == sorted(itertools.product(ends, ends))
    assert all(0 <= D <= 255 and L >= 0 for L, D in ml.CROSS)
    assert len({D // 64 for _, D in ml.CROSS}) == 4
    # the named subsets that go through the Python oracle hold every named tail of both hashes
    assert {ml.b0_tail(L) for L in ml.named_msg_lens()} == set(ml.NAMED)
    assert {ml.bi_tail(D) for D in ml.named_dst_lens()} >= set(ml.NAMED)
    assert {ml.b0_tail(ml.DST_MSG_LEN, D) for D in ml.named_dst_lens()} >= set(ml.NAMED)
    # contents: three per length, of that length; the empty message once
    assert ml.contents(0) == [b""]
    for L in (1, 33, 4099):
        c = ml.contents(L)
        assert [len(m) for m in c] == [L] * 3 and c[0] == bytes(L) and c[1] == b"\xff" * L and len(set(c)) == 3
    assert len(ml.all_cases()) == 3 * (len(ml.MSG_LENS) - 1) + 1 + 256 + 16
    assert set(ml.named_cases()) <= set(ml.all_cases())


def test_expand_message_xmd_equals_the_rfc_restatement():
    for m, dst in ml.all_cases():
        assert h2c.expand_message_xmd(m, dst, 256) == xmd_rfc9380(m, dst), (len(m), len(dst))
    # (the restatement itself against RFC 9380 appendix K.1's first vector)
    k1 = b"QUUX-V01-CS02-with-expander-SHA256-128"
    assert xmd_rfc9380(b"", k1, 32).hex() == "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"
    assert xmd_rfc9380(b"abc", k1, 32).hex() == "d8ccab23b5985ccea865c6c97b6e5b8350e794e603b4b97902f53a8a0d605615"


@pytest.fixture(scope="module")
def c_oracle():
    subprocess.check_call(["make", "-s", "-C", co.CDIR])  # as tests/test_oracle_c.py: rebuilt when stale
    return co.lib()


@pytest.fixture(scope="module")
def python_points():
    """the Python oracle at the named cases, once"""
    return {(m, dst): g2_serialize(h2c.hash_to_g2(m, dst)) for m, dst in ml.named_cases()}


def test_python_oracle_equals_c_oracle(c_oracle, python_points):
    assert len(python_points) >= 90
    for (m, dst), want in python_points.items():
        assert co.hash_to_g2(m, dst) == want, (len(m), len(dst))


@pytest.mark.parametrize("backend", ["elem", "pair"])
def test_hostcheck_hash_to_g2_equals_both_oracles(c_oracle, python_points, backend):
    hc = ctypes.CDLL(build_hostcheck(backend))  # (a missing compiler is an error here, not a skip)
    wrong = []
    for m, dst in ml.all_cases():
        o = ctypes.create_string_buffer(192)
        hc.hc_hash_to_g2(m, len(m), dst, len(dst), o)
        if o.raw != co.hash_to_g2(m, dst) or o.raw != python_points.get((m, dst), o.raw):
            wrong.append((len(m), len(dst)))
    assert not wrong, wrong
