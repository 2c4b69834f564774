"""The kernels whose doubling steps are built on squares, on the device, against the oracle and
against the forms that keep the old formulas.  Every test here needs an MI355X.

* k_miller_fused (its doubling step is ml_dbl_line_sq, lsg_pairing.hpp: 2 products and 7 squares)
  at 1, 5 and 129 sets -- one pair, one item plus one pair, one workgroup plus one item -- through
  lsg_check_batch_partial_rnd with fixed randomizers, some sets masked by a decode error and by an
  infinite key: 576 bytes equal to the oracle's partial and to the A/B library's split kernels
  (LSG_MILLER_FUSED=0: ml_dbl_step_raw + line_eval, the old formulas).  LSG_SLP_ITEMS=0 keeps the
  one-set programs away there, so the named kernel runs at every size.
* Signature membership (k_sig_subgroup: the |x| chain with mixed additions) at 1, 33 and 65 items
  over adversarial points: the non-subgroup points of tests/golden/sig_decode.json (err == 3),
  points of order 13 and 23 on E2 (inside the chain the accumulator meets the identity and +- the
  base) and valid signatures between them, against the oracle's decode.
* hash_to_G2 (its cofactor clearing doubles with proj_dbl) at 1, 33 and 65 messages against the
  oracle.

Key scaling (k_pk_scale: proj_mul_u64_s3 homogeneous throughout) with the edge scalars 1, 2, 3, 4,
5, 7, 8, 2^63, 2^64 - 1, 0x4924924924924924 and 0xdb6db6db6db6db6d is already pinned to the oracle
by tests/test_gpu_rlc_edges.py (test_edge_scalars_shipped: its EDGES hold every one of them, 20
sets through k_pk_scale; test_edge_scalars_one_wave_programs and _4bit_buckets at 513 and 48 sets),
so it is not repeated here; the sets below are scaled by the same scalars on the way."""
import json
import os

import pytest

from oracle import verifier as ov
from oracle.curves import E2, BlstError, g2_compress, g2_serialize
from oracle.fields import R, f12_coeffs
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests.g2points import decode_on_curve, of_order

pytestmark = pytest.mark.gpu
N_KEYS = 64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF_PK = bytes([0x40]) + bytes(95)
SCALARS = [1, 2, 3, 4, 5, 7, 8, 1 << 63, (1 << 64) - 1, 0x4924924924924924, 0xDB6DB6DB6DB6DB6D,
           0xD201000000010001, 0x0101010101010101]
DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def _f12_bytes(f):
    return b"".join(int(c[0]).to_bytes(48, "big") + int(c[1]).to_bytes(48, "big") for c in f12_coeffs(f))


# ---- the fused Miller kernel
@pytest.fixture(scope="module")
def masked129(ctx):
    """129 sets on 129 messages with their randomizers, and the oracle's partial of the first 1, 5
    and 129 of them (computed once, prefix by prefix).  Set 2 does not decode, set 3 has an infinite
    key (pk - pk); so do sets 64 and 127, 128: the last pair of the workgroup and the lone item of
    the second one."""
    n = 129
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    neg = ctx.sk_to_pk([R - sk for sk in sks])
    msgs = [bd.msg("dbl-steps", i) for i in range(n)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
    sets = [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(n)]
    flat = [(pks[i % N_KEYS], msgs[i], sigs[i]) for i in range(n)]
    for i in (2, 127):
        sets[i] = bd.corrupt_truncate(sets[i])
        flat[i] = (flat[i][0], flat[i][1], sets[i][2])
    for i in (3, 64, 128):
        sets[i] = ([pks[i % N_KEYS], neg[i % N_KEYS]], msgs[i], sigs[i])
        flat[i] = (INF_PK, msgs[i], sigs[i])
    rnd = [SCALARS[i % len(SCALARS)] for i in range(n)]
    exp = {k: ov.batch_partial(flat[:k], rnd[:k]) for k in (1, 5, 129)}
    return sets, rnd, {k: (_f12_bytes(f), e) for k, (f, e) in exp.items()}


def _ab(ab_ctx, monkeypatch, call, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return call(ab_ctx)
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("n", [1, 5, 129])
def test_fused_miller_against_the_oracle_and_the_split_kernels(ab_ctx, masked129, monkeypatch, n):
    sets, rnd, exp = masked129
    exp_part, exp_errs = exp[n]
    assert [i for i, e in enumerate(exp_errs) if e] == [i for i in (2, 3, 64, 127, 128) if i < n]
    fused = _ab(ab_ctx, monkeypatch, lambda c: c.batch_partial_rnd(sets[:n], rnd[:n]), LSG_SLP_ITEMS="0")
    launched = [nm for nm, _ in ab_ctx.last_kernel_times()]
    assert "k_miller_fused" in launched and "k_miller_lines" not in launched, launched
    split = _ab(ab_ctx, monkeypatch, lambda c: c.batch_partial_rnd(sets[:n], rnd[:n]), LSG_SLP_ITEMS="0",
                LSG_MILLER_FUSED="0")
    launched = [nm for nm, _ in ab_ctx.last_kernel_times()]
    assert "k_miller_lines" in launched and "k_miller_fused" not in launched, launched
    pair = _ab(ab_ctx, monkeypatch, lambda c: c.batch_partial_rnd(sets[:n], rnd[:n]), LSG_SLP_ITEMS="0",
               LSG_MF_LANES="0")  # the same step over fp2_t
    assert "k_miller_fused_pair" in [nm for nm, _ in ab_ctx.last_kernel_times()]
    part, errs, anyerr = fused
    assert len(part) == 576 and errs == exp_errs and anyerr == any(exp_errs)
    assert part == exp_part
    assert split == fused
    assert pair == fused


# ---- signature membership and hash_to_G2
@pytest.fixture(scope="module")
def adversarial(ctx):
    """65 compressed encodings with the oracle's decode of each (point bytes or None, code): the
    err == 3 cases of the golden file, points of order 13 and 23, and valid signatures"""
    cases = json.load(open(os.path.join(GOLD, "sig_decode.json")))["cases"]
    bad = [bytes.fromhex(c["sig"]) for c in cases if c["err"] == 3 and len(c["sig"]) == 192]
    assert len(bad) >= 8
    seeds = [decode_on_curve(s.hex()) for s in bad]
    small = []
    for q in (13, 23):
        pt = of_order(q, seeds)
        small += [g2_compress(pt), g2_compress(E2.neg(pt)), g2_compress(E2.mul(pt, 2))]
    sks = [interop_secret_key(i) for i in range(8)]
    good = ctx.sign(sks, [bd.msg("dbl-sub", i) for i in range(8)])
    pool = small + bad + good
    # item 0 of order 13, a valid signature last; the kinds interleaved in between
    encs = [pool[(7 * i) % len(pool)] for i in range(64)] + [good[0]]
    encs[0], encs[32], encs[33] = small[0], small[3], bad[0]
    memo = {}

    def decode(b):
        if b not in memo:
            try:
                memo[b] = (g2_serialize(ov.signature_from_bytes(b, True)), 0)
            except BlstError as e:
                memo[b] = (None, e.code)
        return memo[b]
    exp = [decode(b) for b in encs]
    assert exp[0][1] == 3 and exp[32][1] == 3 and exp[33][1] == 3 and exp[64][1] == 0
    return encs, exp


@pytest.mark.parametrize("n", [1, 33, 65])
def test_signature_membership_over_adversarial_points(ctx, ab_ctx, monkeypatch, adversarial, n):
    encs, exp = adversarial
    got = ctx.sig_decode(encs[:n])
    assert "k_sig_subgroup" in [nm for nm, _ in ctx.last_kernel_times()]
    # the chain over fp2_t (k_sig_subgroup_pair) gives the same answers
    twin = _ab(ab_ctx, monkeypatch, lambda c: c.sig_decode(encs[:n]), LSG_FP2_LANES="0")
    assert "k_sig_subgroup_pair" in [nm for nm, _ in ab_ctx.last_kernel_times()]
    assert twin == got
    assert [e for _, e in got] == [e for _, e in exp[:n]]
    assert all(pt == want for (pt, e), (want, _) in zip(got, exp[:n]) if e == 0)


@pytest.mark.parametrize("n", [1, 33, 65])
def test_hash_to_g2_against_the_oracle(ctx, ab_ctx, monkeypatch, n):
    """k_h2c_clear (LSG_SLP_ITEMS=0: packages this small otherwise clear through the one-set
    programs) and the shipped path, against the C restatement of the oracle"""
    msgs = [bd.msg("dbl-h2c", i) for i in range(n)]
    exp = [co.hash_to_g2(m, DST) for m in msgs]
    got = _ab(ab_ctx, monkeypatch, lambda c: c.hash_to_g2(msgs, DST), LSG_SLP_ITEMS="0")
    assert "k_h2c_clear" in [nm for nm, _ in ab_ctx.last_kernel_times()]
    assert got == exp
    assert ctx.hash_to_g2(msgs, DST) == exp
