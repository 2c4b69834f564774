"""k_miller_fused with one Fp2 component per lane (lodestar_amd/csrc/lsg_k_miller.hip on
lsg_fp2_lanes.hpp) against its pair-form twin k_miller_fused_pair (the A/B library with
LSG_MF_LANES=0), the split kernels (LSG_MILLER_FUSED=0) and the oracle, through the exported
partial; and the pieces of the layout only this kernel uses (the Fp2 x Fp leaf, the product by xi,
v on Fp6, the constants) through lsg_check_mf_lanes at the limb extremes.  LSG_SLP_ITEMS=0 keeps
the one-set programs away, so the fused kernel runs at every size.  Every comparison is exact.
Every test here needs an MI355X."""
import itertools

import pytest

from oracle import verifier as ov
from oracle.fields import f12_coeffs, f2_mul
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu
N_KEYS = 64
P, RINV = sp.P, sp.RINV
HI, LO = (1 << 29) + 8, -8  # the closed range of a carried limb
TWINS = {"k_miller_fused": {},
         "k_miller_fused_pair": {"LSG_MF_LANES": "0"},
         "k_miller_lines": {"LSG_MILLER_FUSED": "0"}}
ALL = ("k_miller_fused", "k_miller_fused_pair", "k_miller_lines", "k_slp_items1")


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets132(ctx):
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    msgs = [bd.msg("mf-lanes", i) for i in range(132)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(132)], msgs)
    return [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(132)]


def run(ab_ctx, monkeypatch, kernel, call):
    """call(ab_ctx) under the switches that select `kernel`; checks that it ran and its twins did not"""
    env = dict(TWINS[kernel], LSG_SLP_ITEMS="0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        out = call(ab_ctx)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    launched = [nm for nm, _ in ab_ctx.last_kernel_times()]
    assert kernel in launched and not [nm for nm in ALL if nm != kernel and nm in launched], launched
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 127, 128, 129, 132])
def test_lane_form_against_its_twins(ab_ctx, sets132, monkeypatch, n):
    """one pair, partly filled items, one full workgroup of 32 items, and (129, 132 sets) a 33rd
    item alone in a second workgroup"""
    sets = sets132[:n]
    got = {k: run(ab_ctx, monkeypatch, k, lambda c: c.batch_partial(sets, seed=1000 + n)) for k in TWINS}
    part, errs, anyerr = got["k_miller_fused"]
    assert len(part) == 576 and errs == [0] * n and not anyerr
    assert got["k_miller_fused_pair"] == got["k_miller_fused"]
    assert got["k_miller_lines"] == got["k_miller_fused"]


def _spoiled(sets132, at):
    sets = list(sets132[:8])
    for i in at:
        sets[i] = bd.corrupt_truncate(sets[i])
    return sets


@pytest.mark.parametrize("at", [(4,), (5,), (6,), (7,), (4, 5, 6, 7)], ids=lambda a: "-".join(map(str, a)))
def test_pairs_that_do_not_contribute(ab_ctx, sets132, monkeypatch, at):
    """an undecodable signature at each pair position of the second item, and the whole item"""
    sets = _spoiled(sets132, at)
    got = {k: run(ab_ctx, monkeypatch, k, lambda c: c.batch_partial(sets, seed=77)) for k in TWINS}
    part, errs, anyerr = got["k_miller_fused"]
    assert [i for i, e in enumerate(errs) if e] == list(at) and anyerr
    assert got["k_miller_fused_pair"] == got["k_miller_fused"]
    assert got["k_miller_lines"] == got["k_miller_fused"]
    # and the item's other pairs did contribute: not the partial of the unspoiled batch
    assert part != run(ab_ctx, monkeypatch, "k_miller_fused", lambda c: c.batch_partial(sets132[:8], seed=77))[0]


def _f12_bytes(f):
    return b"".join(int(c[0]).to_bytes(48, "big") + int(c[1]).to_bytes(48, "big") for c in f12_coeffs(f))


@pytest.mark.parametrize("n", [1, 5])
def test_against_the_oracle(ab_ctx, sets132, monkeypatch, n):
    sets = sets132[:n]
    rnd = [0xD201000000010001, 3, 1 << 63, (1 << 64) - 1, 0x0101010101010101][:n]
    f, exp_errs = ov.batch_partial([(p[0], m, s) for p, m, s in sets], rnd)
    part, errs, anyerr = run(ab_ctx, monkeypatch, "k_miller_fused", lambda c: c.batch_partial_rnd(sets, rnd))
    assert errs == exp_errs == [0] * n and not anyerr
    assert part == _f12_bytes(f)


# ---- the hooks
def words(elems):
    return [w for e in elems for w in sp.pair_words(e)]


def fp2_at(out, item, j, per_item=24):
    o = 14 * (per_item * item + 2 * j)
    return sp.from_pair_words(out[o:o + 14]), sp.from_pair_words(out[o + 14:o + 28])


def extremes():
    """every low limb at one end of the carried range, the top limb at both ends of its range;
    the alternating patterns"""
    pats = [sp.clamp([lo] * 13 + [top]) for lo, top in itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX))]
    pats += [sp.clamp([HI if k % 2 else LO for k in range(13)] + [sp.TOP_MAX]),
             sp.clamp([LO if k % 2 else HI for k in range(13)] + [-sp.TOP_MAX])]
    return pats


@pytest.fixture(scope="module")
def leaf_items():
    """65 items (two waves and one pair of a third) of six Fp2 values; A, B, C are read.  Odd
    items take combinations of the extremes, even items seeded patterns; the all-extreme items sit
    in the first and the last lane pair of the first two waves (items 0, 31, 32, 63)"""
    E, f2 = extremes(), sp.fp2_items()
    combos = [(a0, a1) for a0, a1 in itertools.product(E, E)]
    items = []
    for i in range(65):
        items.append([combos[(6 * i + j) % len(combos)] if i % 2 else f2[(6 * i + j) % len(f2)] for j in range(6)])
    for at, (lo, top) in zip((0, 31, 32, 63), itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX))):
        e = sp.clamp([lo] * 13 + [top])
        items[at] = [(e, e), (e, E[at % 6]), (E[(at + 1) % 6], e)] + [(e, e)] * 3
    return items


def test_mul_fp_xi_and_constants_at_the_limb_extremes(ctx, leaf_items):
    n = len(leaf_items)
    assert n == 65
    out = ctx.check_mf_lanes(words(c for it in leaf_items for v in it for c in v))
    for i, it in enumerate(leaf_items):
        (a0, a1), (b0, b1), (c0, c1) = [(sp.value(x0), sp.value(x1)) for x0, x1 in it[:3]]
        Y = [fp2_at(out, i, j) for j in range(11)]
        # Fp2 x Fp: the pair form's words, the oracle's value, normalised limbs
        assert Y[0] == Y[1], i
        A = (a0 * RINV % P, a1 * RINV % P)
        assert tuple(sp.value(x) * RINV % P for x in Y[0]) == f2_mul(A, (b0 * RINV % P, 0)), i
        assert all(0 <= x < (1 << 29) for c in Y[0] for x in c[:13]), i
        # xi, carried and inside a longer sum: the pair form's words, the integers
        assert Y[2] == Y[3] and Y[4] == Y[5], i
        assert (sp.value(Y[2][0]), sp.value(Y[2][1])) == (a0 - a1, a0 + a1), i
        d0, d1 = b0 - c0, b1 - c1
        assert (sp.value(Y[4][0]), sp.value(Y[4][1])) == (a0 + d0 - d1, a1 + d0 + d1), i
        assert all(LO <= x <= HI for y in (Y[2], Y[4]) for c in y for x in c[:13]), i
        # v (A, B, C) = (xi C, A, B)
        assert (sp.value(Y[6][0]), sp.value(Y[6][1])) == (c0 - c1, c0 + c1), i
        assert Y[7] == (list(it[0][0]), list(it[0][1])) and Y[8] == (list(it[1][0]), list(it[1][1])), i
        # the constants: 1 in Montgomery form, 0
        assert sp.value(Y[9][0]) * RINV % P == 1 and Y[9][1] == [0] * 14, i
        assert Y[10] == ([0] * 14, [0] * 14), i
        # the Fp factor as the lanes hold it: all 14 limbs of B.c0 on both lanes
        raw = out[14 * (24 * i + 22):14 * (24 * i + 24)]
        s32 = [x - (1 << 32) if x >= (1 << 31) else x for x in raw]
        assert s32[0::2] == list(it[1][0]) and s32[1::2] == list(it[1][0]), i
