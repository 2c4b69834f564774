"""The random linear combination with randomizers the test chooses (lsg_check_batch_partial_rnd,
Context.batch_partial_rnd): edge scalars through every scaling form, skewed bucket occupancies
through the bucket MSM, per-message key sums, and the forgeries that only distinct randomizers
reject.  Every test here needs an MI355X.

The reference is oracle.verifier.batch_partial on Python integers with the same randomizers,
compared byte for byte (576 bytes, 12 canonical big-endian Fp in tower order), as
tests/test_gpu_parity.py test_batch_partial_bit_exact_vs_oracle does under seeded draws.  Where a
case costs the oracle too much (n = 513, n = 600, most n = 256 patterns) the shipped library is
compared with the A/B library's per-set scaling, which the n = 20 case pins to the oracle for
every edge scalar, and with its bucket MSM.

Scaling forms: the shipped library scales keys with k_pk_scale and the signatures of packages
of up to 2048 sets with k_slp_g2_scale (from 256 sets on the bucket MSM sums them unscaled); the
A/B library (conftest.py ab_ctx) reads LSG_SLP_ITEMS=0 (k_sig_prep scales: k_sig_scale3),
LSG_MSM_MIN_GROUP (1: every group by buckets, 2-bit windows below 48 sets, 4-bit below 256, 8-bit
from there; 1000000: never) and LSG_MSG_AGG=0 (one Miller pair per set) from the environment.
"""
import pytest

from oracle import verifier as ov
from oracle.curves import E2, G2_GEN, g2_compress, g2_uncompress
from oracle.fields import R, f12_coeffs, f12_eq, f12_is_one
from oracle.interop import interop_secret_key
from oracle.pairing import final_exp_fast
from tests import blsdata as bd

pytestmark = pytest.mark.gpu
N_KEYS = 1024
M64 = (1 << 64) - 1
INF96 = bytes([0xC0]) + bytes(95)
NO_MSM = "1000000"

# one per set of the n = 20 case
EDGES = [
    1, 2, 3, 4, 5, 7, 8,
    0x4924924924924924,  # every 3-bit window is 4: each one borrows
    0xDB6DB6DB6DB6DB6D,
    0x2492492492492492,
    1 << 63, (1 << 63) - 1, M64, (1 << 64) - (1 << 32), (1 << 32) - 1,
    0x8000000000000001,
    0xFF00000000000000,
    0x0101010101010101, 0x8080808080808080,
    0xAAAAAAAAAAAAAAAA,  # every 2-bit window is 2
]
assert len(EDGES) == 20 and len(set(EDGES)) == 20


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    return sks, ctx.sk_to_pk(sks)


def single_sets(ctx, keys, tag, n):
    sks, pks = keys
    msgs = [bd.msg(tag, i) for i in range(n)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
    return [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(n)]


def splitmix(seed, n):
    s, out = seed, []
    while len(out) < n:
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        if z:
            out.append(z)
    return out


def _f12_bytes(f):
    return b"".join(int(c[0]).to_bytes(48, "big") + int(c[1]).to_bytes(48, "big") for c in f12_coeffs(f))


def _f12_from_bytes(b):
    assert len(b) == 576
    c = [(int.from_bytes(b[96 * k:96 * k + 48], "big"), int.from_bytes(b[96 * k + 48:96 * k + 96], "big")) for k in range(6)]
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


def oracle_partial(sets, rnd):
    f, errs = ov.batch_partial([(p[0], m, s) for p, m, s in sets], rnd)
    return _f12_bytes(f), errs


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def ab_partial(ab_ctx, monkeypatch, sets, rnd, **env):
    """the A/B library's partial under the given switches (unset again afterwards)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return ab_ctx.batch_partial_rnd(sets, rnd)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def negated_pair(ctx, keys, k, m):
    """Two valid sets on message m whose keys are pk and -pk and whose signatures are sigma and
    -sigma: secret keys sk and r - sk (as tests/test_gpu_sig_groups.py builds its cancelling group)"""
    sk = keys[0][k]
    pks = ctx.sk_to_pk([sk, R - sk])
    sigs = ctx.sign([sk, R - sk], [m, m])
    return ([pks[0]], m, sigs[0]), ([pks[1]], m, sigs[1])


# ---- B1: edge scalars through every scaling form
@pytest.fixture(scope="module")
def edge20(ctx, keys):
    """20 sets, set i scaled by EDGES[i]; set 4 (r = 5) carries the infinity encoding and set 17
    (r = 0x0101...) does not decode (test_edge_scalars_4bit_buckets spoils other positions, so every
    scalar meets a valid signature under the oracle).  The oracle's partial is computed once."""
    sets = single_sets(ctx, keys, "rlc-edge", 20)
    sets[4] = bd.corrupt_infinity(sets[4])
    sets[17] = bd.corrupt_truncate(sets[17])
    exp, errs = oracle_partial(sets, EDGES)
    assert errs == [0] * 17 + [10, 0, 0]
    return sets, exp, errs


def test_edge_scalars_shipped(ctx, edge20):
    sets, exp, exp_errs = edge20
    part, errs, anyerr = ctx.batch_partial_rnd(sets, EDGES)
    launched = names(ctx)
    assert "k_pk_scale" in launched and "k_slp_g2_scale" in launched and "msm_buckets" not in launched
    assert errs == exp_errs and anyerr
    assert part == exp
    # the hook is lsg_batch_partial with other randomizers: the seeded draws give the seeded bytes
    assert ctx.batch_partial_rnd(sets, splitmix(77, 20)) == ctx.batch_partial(sets, seed=77)


def test_edge_scalars_serial_scaling(ab_ctx, edge20, monkeypatch):
    sets, exp, exp_errs = edge20
    part, errs, anyerr = ab_partial(ab_ctx, monkeypatch, sets, EDGES, LSG_SLP_ITEMS="0", LSG_MSM_MIN_GROUP=NO_MSM)
    launched = names(ab_ctx)
    assert "k_sig_prep" in launched and "k_slp_g2_scale" not in launched and "msm_buckets" not in launched
    assert errs == exp_errs and anyerr
    assert part == exp


def test_edge_scalars_2bit_buckets(ab_ctx, edge20, monkeypatch):
    sets, exp, exp_errs = edge20
    part, errs, anyerr = ab_partial(ab_ctx, monkeypatch, sets, EDGES, LSG_MSM_MIN_GROUP="1")
    assert "msm_buckets" in names(ab_ctx)
    assert errs == exp_errs and anyerr
    assert part == exp


def test_edge_scalars_4bit_buckets(ctx, ab_ctx, keys, monkeypatch):
    """48 sets, the smallest group with 4-bit windows, the list cycled; an infinite and an
    undecodable signature at other scalars than in the 20-set case."""
    n = 48
    sets = single_sets(ctx, keys, "rlc-edge48", n)
    rnd = [EDGES[i % 20] for i in range(n)]
    sets[26] = bd.corrupt_infinity(sets[26])   # r = 8
    sets[42] = bd.corrupt_truncate(sets[42])   # r = 3
    exp, exp_errs = oracle_partial(sets, rnd)
    part, errs, anyerr = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP="1")
    assert "msm_buckets" in names(ab_ctx)
    assert errs == exp_errs and anyerr and errs[42] == 10
    assert part == exp
    assert ctx.batch_partial_rnd(sets, rnd)[0] == exp  # and the shipped per-set programs


def test_edge_scalars_one_wave_programs(ctx, ab_ctx, keys, monkeypatch):
    """513 sets, the smallest package past 512 program items, where the straight-line programs
    run their one-wave schedule (lsg_slp.hip slp_waves), the list cycled.  The shipped library
    (programs for the subgroup checks and Miller items, buckets for the signature sum) against
    the A/B library's serial scaling, which the 20-set case pins to the oracle per scalar; the
    one-wave k_slp_g2_scale itself runs in the A/B library with the buckets off."""
    n = 513
    sets = single_sets(ctx, keys, "rlc-edge513", n)
    rnd = [EDGES[i % 20] for i in range(n)]
    part, errs, anyerr = ctx.batch_partial_rnd(sets, rnd)
    assert errs == [0] * n and not anyerr
    ref, rerrs, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_SLP_ITEMS="0", LSG_MSM_MIN_GROUP=NO_MSM)
    assert "k_slp_g2_scale" not in names(ab_ctx) and "msm_buckets" not in names(ab_ctx)
    assert rerrs == errs
    assert part == ref
    # the programs' own scaling at this size (A/B library: no buckets, programs on)
    slp, _, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP=NO_MSM)
    assert "k_slp_g2_scale" in names(ab_ctx)
    assert slp == ref
    assert ab_ctx.final_verify([ref])


# ---- B2: skewed bucket MSM
N_SKEW = (256, 600)
ONE_PASS_MAX = 32 * 16  # members of one chunk: 32 lane pairs x SEG_FOLD (lsg_plan.hpp)


@pytest.fixture(scope="module")
def skew_sets(ctx, keys):
    """600 valid sets on distinct messages (the 256-set cases take the first 256), and the pair
    that the "cancel" pattern puts at sets 10 and 11: sigma and -sigma on one message under keys
    pk and -pk, both valid"""
    return single_sets(ctx, keys, "rlc-skew", 600), negated_pair(ctx, keys, 700, bd.msg("rlc-skew-neg", 0))


PATTERNS = ("all_equal", "top_bit", "one", "all_ones", "one_window", "window_per_set", "half_ones", "cancel")


def skew_patterns(n):
    draws = splitmix(0xB2, n)
    cancel = list(draws)
    cancel[11] = cancel[10]  # sigma and -sigma with equal randomizers: one bucket sum passes through infinity
    return {
        "all_equal": [0x0101010101010101] * n,                          # 8 buckets hold all n sets, 2032 are empty
        "top_bit": [1 << 63] * n,                                       # one bit sum non-empty
        "one": [1] * n,
        "all_ones": [M64] * n,                                          # bucket 255 of every window holds all sets
        "one_window": [(1 + i % 255) << 24 for i in range(n)],          # every bucket of window 3, no other
        "window_per_set": [(1 + i % 255) << (8 * (i % 8)) for i in range(n)],
        "half_ones": [M64 if i % 2 else draws[i] for i in range(n)],
        "cancel": cancel,
    }


@pytest.mark.parametrize("n", N_SKEW)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_skewed_buckets_match_scalar_path(ctx, ab_ctx, skew_sets, monkeypatch, n, pattern):
    sets = skew_sets[0][:n]
    if pattern == "cancel":
        sets[10], sets[11] = skew_sets[1]
    rnd = skew_patterns(n)[pattern]
    assert sorted(skew_patterns(n)) == sorted(PATTERNS) and all(0 < r <= M64 for r in rnd)
    scalar, errs, anyerr = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP=NO_MSM)
    assert "msm_buckets" not in names(ab_ctx)
    assert errs == [0] * n and not anyerr
    assert ab_ctx.final_verify([scalar]), "the sets are valid: the reference partial must pass"
    msm, _, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP="1")
    assert "msm_buckets" in names(ab_ctx)
    assert msm == scalar
    part, errs, anyerr = ctx.batch_partial_rnd(sets, rnd)
    launched = names(ctx)
    assert errs == [0] * n and not anyerr
    assert part == scalar
    if pattern in ("all_equal", "top_bit", "one", "all_ones"):
        # a bucket of n members: a second pass past one chunk, and only then
        assert launched.count("msm_buckets") == (2 if n > ONE_PASS_MAX else 1), launched
    else:
        assert "msm_buckets" in launched


def test_signature_sum_at_infinity(ctx, ab_ctx, keys, monkeypatch):
    """256 sets whose signature sum is the point at infinity, ML(-G1, O) = 1: sets 0 and 1 are
    sigma and -sigma with equal randomizers, every other signature is the infinity encoding.  So
    that the package is still valid (and the check is one the final exponentiation decides), the
    other 254 sets come in pairs on one message under keys pk and -pk with equal randomizers:
    e(r pk, H) e(-r pk, H) = 1.  With per-message key sums every message's sum is infinity
    (k_pk_mask, k_g1p_affine_inv's pinf); LSG_MSG_AGG=0 pairs every set on its own."""
    n = 256
    sets = list(negated_pair(ctx, keys, 701, bd.msg("rlc-inf", 0)))
    for j in range(1, n // 2):
        a, b = negated_pair(ctx, keys, j, bd.msg("rlc-inf", j))
        sets += [(a[0], a[1], INF96), (b[0], b[1], INF96)]
    draws = splitmix(0x1F, n // 2)
    rnd = [draws[i // 2] for i in range(n)]
    scalar, errs, anyerr = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP=NO_MSM)
    assert errs == [0] * n and not anyerr
    assert ab_ctx.final_verify([scalar])
    msm, _, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP="1")
    assert msm == scalar
    part, errs, anyerr = ctx.batch_partial_rnd(sets, rnd)
    launched = names(ctx)
    assert "msm_buckets" in launched and "k_pk_mask" in launched
    assert errs == [0] * n and not anyerr
    assert part == scalar
    per_set, _, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSM_MIN_GROUP="1", LSG_MSG_AGG="0")
    assert "k_pk_mask" not in names(ab_ctx)
    assert ab_ctx.final_verify([per_set])
    # distinct randomizers inside the pairs: nothing cancels any more
    assert not ctx.final_verify([ctx.batch_partial_rnd(sets, splitmix(0x2F, n))[0]])


def test_half_ones_256_bit_exact_vs_oracle(ctx, ab_ctx, skew_sets, monkeypatch):
    """One skewed pattern pinned to the oracle bit for bit (about 10 s of CPU)."""
    import time
    n = 256
    sets = skew_sets[0][:n]
    rnd = skew_patterns(n)["half_ones"]
    t0 = time.time()
    exp, exp_errs = oracle_partial(sets, rnd)
    print("oracle batch_partial, n = 256: %.1f s" % (time.time() - t0))
    part, errs, anyerr = ctx.batch_partial_rnd(sets, rnd)
    assert "msm_buckets" in names(ctx)
    assert errs == exp_errs == [0] * n and not anyerr
    assert part == exp


# ---- B3: per-message key sums
def _msg_sum_sets(ctx, keys):
    """six sets on two messages: message A under keys pk and -pk (its key sum is infinity under
    equal randomizers), message B under four keys"""
    sks, pks = keys
    ma, mb = bd.msg("rlc-magg", 0), bd.msg("rlc-magg", 1)
    a, b = negated_pair(ctx, keys, 40, ma)
    sigs = ctx.sign([sks[41 + k] for k in range(4)], [mb] * 4)
    sets = [a, b] + [([pks[41 + k]], mb, sigs[k]) for k in range(4)]
    rnd = [7, 7, 3, 0x8000000000000001, M64, 1]
    return sets, rnd


@pytest.mark.parametrize("forged", [False, True], ids=["valid", "one-forged"])
def test_message_key_sums_against_oracle(ctx, ab_ctx, keys, monkeypatch, forged):
    """e(sum r_i pk_i, H(m)) is not bit-identical to the per-set product: the oracle's final
    exponentiation of the device partial equals that of the oracle's partial.  With set 3 carrying
    set 4's signature the common value is not one, so the comparison is of a whole GT element."""
    sets, rnd = _msg_sum_sets(ctx, keys)
    if forged:
        sets[3] = (sets[3][0], sets[3][1], sets[4][2])
    f, exp_errs = ov.batch_partial([(p[0], m, s) for p, m, s in sets], rnd)
    want = final_exp_fast(f)
    assert f12_is_one(want) == (not forged)
    part, errs, anyerr = ctx.batch_partial_rnd(sets, rnd)
    launched = names(ctx)
    assert "k_pk_mask" in launched and "k_g1p_affine_inv" in launched and "k_slp_items_msg" in launched
    assert errs == exp_errs == [0] * 6 and not anyerr
    assert part != _f12_bytes(f)  # two pairs instead of six: other bytes, the same class
    assert f12_eq(final_exp_fast(_f12_from_bytes(part)), want)
    assert ctx.final_verify([part]) == (not forged)
    # one pair per set (A/B library): the oracle's own product, byte for byte
    per_set, errs, _ = ab_partial(ab_ctx, monkeypatch, sets, rnd, LSG_MSG_AGG="0")
    assert "k_pk_mask" not in names(ab_ctx)
    assert errs == exp_errs
    assert per_set == _f12_bytes(f)


# ---- B4: the forgeries of tests/test_gpu_rlc_forgeries.py are real, and only the randomizers reject them
def offset_pair(a, b):
    """sig_a + D and sig_b - D: each set invalid, the unrandomised sum valid"""
    D = E2.mul(G2_GEN, 123456789)
    sa = E2.add(g2_uncompress(a[2]), D)
    sb = E2.add(g2_uncompress(b[2]), E2.neg(D))
    return (a[0], a[1], g2_compress(sa)), (b[0], b[1], g2_compress(sb))


def swapped_pair(ctx, keys, ka, kb, m):
    """(pk_a, m, sig_b) and (pk_b, m, sig_a): each set invalid, the unrandomised product valid"""
    sks, pks = keys
    sa, sb = ctx.sign([sks[ka], sks[kb]], [m, m])
    return ([pks[ka]], m, sb), ([pks[kb]], m, sa)


@pytest.mark.parametrize("kind", ["offset", "swap"])
@pytest.mark.parametrize("n_valid", [0, 256], ids=["alone", "among-256"])
def test_cancelling_forgery_needs_distinct_randomizers(ctx, ab_ctx, keys, monkeypatch, kind, n_valid):
    from tests import cpu_oracle as co
    if kind == "offset":
        fa, fb = offset_pair(*single_sets(ctx, keys, "rlc-b4", 2))
    else:
        fa, fb = swapped_pair(ctx, keys, 5, 6, bd.msg("rlc-b4-swap", 0))
    assert co.verify_each([fa[0][0], fb[0][0]], [fa[1], fb[1]], [fa[2], fb[2]]) == [0, 0]
    valid = single_sets(ctx, keys, "rlc-b4-valid", n_valid)
    at = (0, 1) if not n_valid else (100, 201)
    sets = list(valid)
    sets.insert(at[0], fa)
    sets.insert(at[1], fb)
    n = len(sets)
    draws = splitmix(0xB4, n)
    equal = list(draws)
    equal[at[1]] = equal[at[0]]
    for c in (ctx, ab_ctx):
        part, errs, anyerr = c.batch_partial_rnd(sets, equal)
        assert errs == [0] * n and not anyerr
        assert ("msm_buckets" in names(c)) == (n >= 256)
        assert c.final_verify([part]), "equal randomizers: the forged pair cancels"
        part, _, _ = c.batch_partial_rnd(sets, draws)
        assert not c.final_verify([part]), "distinct randomizers reject it"
    if n_valid:  # the per-set scaling path agrees
        part, _, _ = ab_partial(ab_ctx, monkeypatch, sets, equal, LSG_MSM_MIN_GROUP=NO_MSM)
        assert ab_ctx.final_verify([part])
        part, _, _ = ab_partial(ab_ctx, monkeypatch, sets, draws, LSG_MSM_MIN_GROUP=NO_MSM)
        assert not ab_ctx.final_verify([part])


# ---- B5: arguments
def test_hook_arguments(ctx, keys):
    import ctypes
    from lodestar_amd._native import Context, SetBuffer, LSG_ERR_INVALID_ARG
    sets = single_sets(ctx, keys, "rlc-args", 3)
    b = SetBuffer(sets)
    rnd = (ctypes.c_uint64 * 3)(5, 6, 7)
    zero = (ctypes.c_uint64 * 3)(5, 0, 7)
    out = ctypes.create_string_buffer(576)
    errs = (ctypes.c_int32 * 3)()
    anyerr = ctypes.c_int32()
    fn = ctx.lib.lsg_check_batch_partial_rnd
    good = ctx.batch_partial_rnd(sets, [5, 6, 7])
    assert ctx.final_verify([good[0]])
    for args in ((None, b.arr, 3, rnd, out, errs, ctypes.byref(anyerr)),
                 (ctx.h, None, 3, rnd, out, errs, ctypes.byref(anyerr)),
                 (ctx.h, b.arr, 3, None, out, errs, ctypes.byref(anyerr)),
                 (ctx.h, b.arr, 3, rnd, None, errs, ctypes.byref(anyerr)),
                 (ctx.h, b.arr, 3, rnd, out, errs, None),
                 (ctx.h, b.arr, 3, zero, out, errs, ctypes.byref(anyerr))):
        assert fn(*args) == LSG_ERR_INVALID_ARG
        assert ctx.batch_partial_rnd(sets, [5, 6, 7]) == good  # the context stays usable
    assert fn(ctx.h, b.arr, 3, rnd, out, None, ctypes.byref(anyerr)) == 0 and out.raw == good[0]  # set_err is optional
    with pytest.raises(RuntimeError, match=r"\(%d\)" % LSG_ERR_INVALID_ARG):
        ctx.batch_partial_rnd(sets, [5, 0, 7])
    c2 = Context(devices=[0, 0])
    try:
        with pytest.raises(RuntimeError, match=r"\(%d\)" % LSG_ERR_INVALID_ARG):
            c2.batch_partial_rnd(sets, [5, 6, 7])
        assert c2.verify_sets(sets, seed=3) == (1, 0)
    finally:
        c2.close()
    assert ctx.batch_partial_rnd(sets, [5, 6, 7]) == good
