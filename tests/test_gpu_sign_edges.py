"""k_sign and k_sk_to_pk (lsg_sign, lsg_sk_to_pk) against the oracle at edge scalars.  The two
kernels make the inputs of most GPU tests and of the soak, and were compared with the oracle only
through interop keys; here directly, byte for byte, at scalars where a 256-bit double-and-add
goes wrong: 0, the group order and its neighbours and double (the accumulator passes through
infinity, or meets the base point), single bits at byte and word borders, the top bit, all ones,
alternating bits.  Scalars are reduced by nobody on the way in: [k]P = [k mod r]P.
Every test here needs an MI355X."""
import functools

import pytest

from oracle import hash_to_curve as h2c
from oracle.curves import E1, E2, G1_GEN, g1_serialize, g2_compress
from oracle.fields import R
from oracle.interop import interop_secret_key
from tests import msglens as ml

pytestmark = pytest.mark.gpu
G1_INF = bytes([0x40]) + bytes(95)
G2_INF = bytes([0xC0]) + bytes(95)


def _scalars():
    ks = [0, 1, 2, R - 1, R, R + 1, 2 * R, 1 << 255, (1 << 256) - 1]
    ks += [1 << k for k in (0, 7, 8, 63, 64, 127, 128, 254, 255)]
    ks += [int.from_bytes(b"\x55" * 32, "big"), int.from_bytes(b"\xaa" * 32, "big")]
    ks += [interop_secret_key(i) for i in range(8)]
    assert all(0 <= k < (1 << 256) for k in ks)
    return list(dict.fromkeys(ks))  # (2^0 and 2^255 are listed twice)


SCALARS = _scalars()
# 65 items: two full waves of the one-item-per-lane-pair launch and one item of a third; every
# scalar is there, at changing places
SCALARS65 = [SCALARS[(7 * i) % len(SCALARS)] for i in range(65)]
MSGS = {32: [ml.rnd_msg(32, salt=40 + j) for j in range(3)], 9: [ml.rnd_msg(9, salt=40 + j) for j in range(3)]}


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def pk_of(k):
    return g1_serialize(E1.mul(G1_GEN, k % R) if k % R else None)


@functools.lru_cache(maxsize=None)
def h_of(m):
    return h2c.hash_to_g2(m)


@functools.lru_cache(maxsize=None)
def sig_of(k, m):
    return g2_compress(E2.mul(h_of(m), k % R) if k % R else None)


def test_the_scalar_list():
    assert len(SCALARS) == 26 and set(SCALARS65) == set(SCALARS)
    assert [k for k in SCALARS if k % R == 0] == [0, R, 2 * R]
    assert {R - 1, R + 1, 1 << 255, (1 << 256) - 1, 1 << 7, 1 << 8, 1 << 63, 1 << 64, 1 << 127, 1 << 128, 1 << 254} <= set(SCALARS)
    assert len({SCALARS65[i] for i in (0, 31, 32, 63, 64)}) == 5  # the wave borders hold different scalars
    assert pk_of(0) == pk_of(R) == G1_INF == g1_serialize(None)
    assert sig_of(2 * R, MSGS[9][0]) == G2_INF == g2_compress(None)


def test_sk_to_pk_one_scalar_per_launch(ctx):
    for k in SCALARS:
        assert ctx.sk_to_pk([k]) == [pk_of(k)], hex(k)


def test_sk_to_pk_65_scalars(ctx):
    got = ctx.sk_to_pk(SCALARS65)
    wrong = [(i, hex(k)) for i, (k, g) in enumerate(zip(SCALARS65, got)) if g != pk_of(k)]
    assert not wrong and len(got) == 65, wrong
    assert [g for k, g in zip(SCALARS65, got) if k % R == 0] == [G1_INF] * sum(1 for k in SCALARS65 if k % R == 0)


@pytest.mark.parametrize("length", [32, 9])
def test_sign_one_scalar_per_launch(ctx, length):
    m = MSGS[length][0]
    for k in SCALARS:
        assert ctx.sign([k], [m]) == [sig_of(k, m)], hex(k)


@pytest.mark.parametrize("length", [32, 9])
def test_sign_65_scalars(ctx, length):
    msgs = [MSGS[length][i % 3] for i in range(65)]
    got = ctx.sign(SCALARS65, msgs)
    wrong = [(i, hex(k)) for i, (k, m, g) in enumerate(zip(SCALARS65, msgs, got)) if g != sig_of(k, m)]
    assert not wrong and len(got) == 65, wrong
    assert [g for k, g in zip(SCALARS65, got) if k % R == 0] == [G2_INF] * sum(1 for k in SCALARS65 if k % R == 0)
