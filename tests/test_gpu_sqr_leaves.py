"""The squaring leaves of the pair backend on the device (lodestar_amd/csrc/lsg_fp_pair.hpp:
pair_mont_sqr behind fp_sqr, pair_fp2_sqr_v behind fp2_sqr, the squarings of pair_pow_plan)
at the lazy bounds of their inputs: limbs at -8, 2^29 + 7 and 0, alternating extremes, signed
top limbs with |v| < 2^12.6 p, seeded random patterns (tests/sqr_patterns.py), against Python
integers, the product leaf and the oracle.  lsg_check_fp_sqr / lsg_check_fp2_sqr run the leaves
the kernels call.  Every test here needs an MI355X."""
import ctypes

import pytest

from tests import cpu_oracle as co
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu
P, RINV = sp.P, sp.RINV


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def test_fp_sqr_is_the_product_leaf_bit_for_bit(ctx):
    """(a) fp_sqr(a) equals, word for word, the c0 of the Fp2 product leaf on (a, 0)(a, 0) -- the
    same accumulated integer a a + sum m_s p 2^(29 s) through the same tail -- is a^2 / 2^406
    mod p, and has limbs 0..12 in [0, 2^29)."""
    items = sp.fp_items()
    assert len(items) == 312
    zero = [0] * 14
    out = ctx.check_fp_sqr([w for a in items for w in sp.pair_words(a)])
    ref = ctx.check_fp2_mul([w for a in items for e in (a, zero, a, zero) for w in sp.pair_words(e)])
    for i, a in enumerate(items):
        got = out[14 * i:14 * i + 14]
        assert got == ref[28 * i:28 * i + 14], i
        limbs = sp.from_pair_words(got)
        va = sp.value(a)
        assert (sp.value(limbs) - va * va * RINV) % P == 0, i
        assert all(0 <= c < (1 << 29) for c in limbs[:13]), i


def test_fp2_sqr_values_bound_and_normalised_limbs(ctx):
    """(b) c0 = (a0^2 - a1^2) / 2^406, c1 = 2 a0 a1 / 2^406 mod p, |out| < 3p, limbs 0..12 in
    [0, 2^29) (the operands a0 + a1, a0 - a1 and a1 + a1 enter the products without a carry
    round: columns of 7 terms below 2^59.1 and 7 below 2^58 per lane)."""
    items = sp.fp2_items()
    assert len(items) == 312
    out = ctx.check_fp2_sqr([w for it in items for e in it for w in sp.pair_words(e)])
    for i, (a0, a1) in enumerate(items):
        v0, v1 = sp.value(a0), sp.value(a1)
        c0, c1 = sp.from_pair_words(out[28 * i:28 * i + 14]), sp.from_pair_words(out[28 * i + 14:28 * i + 28])
        w0, w1 = sp.value(c0), sp.value(c1)
        assert (w0 - (v0 * v0 - v1 * v1) * RINV) % P == 0, i
        assert (w1 - 2 * v0 * v1 * RINV) % P == 0, i
        assert abs(w0) < 3 * P and abs(w1) < 3 * P, i
        assert all(0 <= c < (1 << 29) for c in c0[:13] + c1[:13]), i


def test_fixed_exponent_powers_still_agree_with_the_oracle(ctx):
    """(c) The same inputs reduced below p as the x coordinates of compressed signatures: the
    square-root powers of ctx.sig_decode (with 33 valid signatures: full waves and a partial
    one) give the C oracle's error code and point; and one verify_sets call of 33 sets -- a wave
    of 32 items plus one -- has the oracle's verdict, valid and with one wrong message."""
    import hashlib
    from oracle.interop import interop_secret_key
    from tests import blsdata as bd
    n = 33
    sks = [interop_secret_key(i) for i in range(n)]
    pks = ctx.sk_to_pk(sks)
    msgs = [hashlib.sha256(b"lodestar-mi355x" + b"sqr-leaves" + i.to_bytes(8, "little")).digest() for i in range(n)]
    sets = [([pks[i]], msgs[i], s) for i, s in enumerate(ctx.sign(sks, msgs))]

    L = co.lib()
    L.cpu_sig_decode.restype = ctypes.c_int
    L.cpu_sig_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    sigs = []
    for k, (a0, a1) in enumerate(sp.fp2_items()):
        b = bytearray((sp.value(a1) % P).to_bytes(48, "big") + (sp.value(a0) % P).to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if k % 2 else 0)  # compressed; either sign of y
        sigs.append(bytes(b))
    sigs += [s for _, _, s in sets]  # points of the group among them: 345 items, 10 waves and 25 pairs
    got = ctx.sig_decode(sigs)
    for k, (s, (pt, err)) in enumerate(zip(sigs, got)):
        want = ctypes.create_string_buffer(192)
        werr = L.cpu_sig_decode(s, 96, want)
        assert err == werr, (k, err, werr)
        if werr == 0:
            assert pt == want.raw, k
    # x off the curve (no root), on it outside the group, and in the group
    assert sorted(set(e for _, e in got)) == [0, 2, 3]

    bad = list(sets)
    bad[32] = bd.corrupt_wrong_message(bad[32])  # the set on the partial wave
    for ss, want in ((sets, [1] * n), (bad, [1] * 32 + [0])):
        per = co.verify_each([p[0] for p, _, _ in ss], [m for _, m, _ in ss], [s for _, _, s in ss])
        assert per == want, per
        assert ctx.verify_sets(ss, seed=5) == ((1, 0) if all(per) else (0, 0))
