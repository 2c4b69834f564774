"""The Fp2 layout with one component per lane (lodestar_amd/csrc/lsg_fp2_lanes.hpp) on the
device: its leaves and linear operations through lsg_check_fp2_lanes / lsg_check_g2_lanes at the
limb extremes, and the two kernels whose [x] chains run in it -- k_sig_subgroup (the whole chain)
through lsg_sig_decode, k_h2c_clear (the chains' doublings) through lsg_check_map_uniform and
lsg_hash_to_g2 -- against their pair-form twins (the A/B library with LSG_FP2_LANES=0) and the
oracle.  Every comparison is exact.
Every test here needs an MI355X."""
import ctypes
import itertools
import json
import os

import pytest

from oracle import hash_to_curve as h2c
from oracle.curves import E2, g2_compress, g2_serialize, g2_uncompress
from oracle.fields import f2_mul, f2_sqr
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import field_edges as fe
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu
P, RINV = sp.P, sp.RINV
R = 1 << 406
HI, LO = (1 << 29) + 8, -8  # the closed range of a carried limb
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


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
    """items of six Fp2 values (A..F).  A wave holds 32 items: the all-extreme items sit in the
    first and the last lane pair of the first two waves (items 0, 31, 32, 63), the other
    combinations of the extremes and the seeded patterns around them; 65 items: a partial wave"""
    E, f2 = extremes(), sp.fp2_items()
    combos = [(a0, a1) for a0, a1 in itertools.product(E, E)]
    items = []
    for i in range(65):
        six = [combos[(6 * i + j) % len(combos)] if i % 2 else f2[(6 * i + j) % len(f2)] for j in range(6)]
        items.append(six)
    for at, (lo, top) in zip((0, 31, 32, 63), itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX))):
        e = sp.clamp([lo] * 13 + [top])
        items[at] = [(e, e)] * 3 + [(E[(at + 1) % 6], e), (e, E[at % 6]), (e, e)]
    return items


def test_leaves_and_sums_at_the_limb_extremes(ctx, leaf_items):
    n = len(leaf_items)
    out = ctx.check_fp2_lanes(words(c for it in leaf_items for v in it for c in v))
    old_mul = ctx.check_fp2_mul(words(c for it in leaf_items for v in it[:2] for c in v))
    old_sqr = ctx.check_fp2_sqr(words(c for it in leaf_items for c in it[0]))
    for i, it in enumerate(leaf_items):
        val = [(sp.value(c0), sp.value(c1)) for c0, c1 in it]
        (a0, a1), (b0, b1) = val[0], val[1]
        Y = [fp2_at(out, i, j) for j in range(11)]
        assert Y[0] == (list(it[0][0]), list(it[0][1])), i  # in and out: the same words
        # the product and the square: the pair-form leaves' words, the oracle's values
        assert words(Y[1]) == old_mul[28 * i:28 * i + 28], i
        assert words(Y[2]) == old_sqr[28 * i:28 * i + 28], i
        A, B = (a0 * RINV % P, a1 * RINV % P), (b0 * RINV % P, b1 * RINV % P)
        assert tuple(sp.value(x) * RINV % P for x in Y[1]) == f2_mul(A, B), i
        assert tuple(sp.value(x) * RINV % P for x in Y[2]) == f2_sqr(A), i
        assert all(0 <= x < (1 << 29) for y in Y[1:3] for c in y for x in c[:13]), i
        # linear operations keep the integer and leave carried limbs
        want = {3: tuple(val[0][c] + val[1][c] + val[2][c] - val[3][c] - val[4][c] - val[5][c] for c in range(2)),
                4: (2 * a0, 2 * a1), 5: (3 * a0, 3 * a1), 6: (4 * a0, 4 * a1), 7: (8 * a0, 8 * a1),
                8: (12 * a0, 12 * a1), 9: (12 * (a0 - a1), 12 * (a0 + a1)), 10: (-a0, -a1)}
        for j, w in want.items():
            assert (sp.value(Y[j][0]), sp.value(Y[j][1])) == w, (i, j)
            assert all(LO <= x <= HI for c in Y[j] for x in c[:13]), (i, j)
        # the lane layout itself: lane 0 (even) holds c0's 14 limbs, lane 1 (odd) c1's
        raw = out[14 * (24 * i + 22):14 * (24 * i + 24)]
        s32 = [x - (1 << 32) if x >= (1 << 31) else x for x in raw]
        assert s32[0::2] == list(it[0][0]) and s32[1::2] == list(it[0][1]), i
    assert n == 65


def _mont(x):
    return fe.norm_limbs(x * R % P)


def _g2_points():
    pts = [g2_uncompress(bytes.fromhex(h)) for h in json.load(open(os.path.join(GOLDEN, "mainnet_g2_points.json")))]
    assert len(pts) >= 8
    return pts


def test_jacobian_doubling_and_addition_in_both_layouts(ctx):
    """jac_dbl and jac_add_proj on mainnet G2 points (Z = 1, then the doubled point as J): the
    lane layout's words are the pair layout's, and the points the oracle's"""
    pts = _g2_points()
    one, zero = (1, 0), (0, 0)
    cases = []
    for k in range(33):  # a full wave and one item
        A, Q = pts[k % len(pts)], pts[(k + 1 + k // len(pts)) % len(pts)]
        if k % 11 == 5:
            Q = A  # J + Q with Q = J: the doubling inside the complete addition
        cases.append((A, Q, (A[0], A[1], one), (Q[0], Q[1], one)))
    A, Q = pts[0], pts[1]
    cases.append((None, Q, (one, one, zero), (Q[0], Q[1], one)))   # J at infinity
    cases.append((A, None, (A[0], A[1], one), (zero, one, zero)))  # Q at infinity
    out = ctx.check_g2_lanes(words(_mont(c) for _, _, J, Qh in cases for v in J + Qh for c in v))

    def jac_affine(X, Y, Z):
        X, Y, Z = (tuple(sp.value(c) * RINV % P for c in v) for v in (X, Y, Z))
        if Z == (0, 0):
            return None
        F = E2.F
        zi = F.inv(Z)
        zi2 = F.sqr(zi)
        return (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi)))
    for i, (A, Q, _, _) in enumerate(cases):
        Y = [fp2_at(out, i, j) for j in range(12)]
        assert Y[0:3] == Y[3:6], i
        assert Y[6:9] == Y[9:12], i
        assert jac_affine(*Y[0:3]) == E2.dbl(A), i
        assert jac_affine(*Y[6:9]) == E2.add(A, Q), i


def _sig_cases():
    """compressed encodings with their expected codes from the C oracle: mainnet G2 points (0),
    points of the curve outside the group (3), encodings in error before the subgroup check (1,
    2: the kernel returns early for the pair), the point at infinity (0, infinite: early too)"""
    gold = json.load(open(os.path.join(GOLDEN, "sig_decode.json")))["cases"]
    c96 = [bytes.fromhex(c["sig"]) for c in gold if len(c["sig"]) == 192]
    good = [bytes.fromhex(h) for h in json.load(open(os.path.join(GOLDEN, "mainnet_g2_points.json")))]
    out3 = [s for s, c in zip(c96, (c for c in gold if len(c["sig"]) == 192)) if c["err"] == 3]
    early = [s for s, c in zip(c96, (c for c in gold if len(c["sig"]) == 192)) if c["err"] in (1, 2)]
    inf = bytes([0xc0]) + bytes(95)
    assert good and out3 and early
    return good, out3, early + [inf]


@pytest.mark.parametrize("n", [1, 32, 33, 65])
def test_sig_subgroup_kernel_against_pair_form_and_oracle(ctx, ab_ctx, monkeypatch, n):
    good, out3, early = _sig_cases()
    if n == 1:
        batches = [[good[0]], [out3[0]], [early[-1]]]
    else:  # a mix that puts every kind in the first and in the last pair of a wave
        kinds = [good, out3, early]
        batches = [[kinds[(i + r) % 3][(i // 3 + r) % len(kinds[(i + r) % 3])] for i in range(n)] for r in range(3)]
    L = co.lib()
    L.cpu_sig_decode.restype = ctypes.c_int
    L.cpu_sig_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    seen = set()
    for sigs in batches:
        got = ctx.sig_decode(sigs)
        assert "k_sig_subgroup" in [nm for nm, _ in ctx.last_kernel_times()]
        monkeypatch.setenv("LSG_FP2_LANES", "0")
        old = ab_ctx.sig_decode(sigs)
        assert "k_sig_subgroup_pair" in [nm for nm, _ in ab_ctx.last_kernel_times()]
        monkeypatch.delenv("LSG_FP2_LANES")
        assert [e for _, e in got] == [e for _, e in old]
        for k, (s, (pt, err)) in enumerate(zip(sigs, got)):
            want = ctypes.create_string_buffer(192)
            werr = L.cpu_sig_decode(s, 96, want)
            assert err == werr, (n, k, err, werr)
            if werr == 0:
                assert pt == want.raw == old[k][0], (n, k)
            seen.add(err)
    assert {0, 3} <= seen


def _clear_names(c):
    return [nm for nm, _ in c.last_kernel_times()]


@pytest.mark.parametrize("n", [1, 33, 65])
def test_h2c_clear_kernel_on_the_map_edges(ab_ctx, monkeypatch, n):
    """lsg_check_map_uniform on the kernel path: u = 0, u1 = u0 (a doubling inside the sum),
    u1 = -u0 (the identity: the chains run on the point at infinity) among seeded inputs"""
    monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    if n == 1:
        table = fe.map_table(33)
        at = [0, 8, 11]  # u0 = 0; u1 = u0; u1 = -u0
        assert table[11][1][0] & 0x40 and not table[8][1][0] & 0x40
        runs = [[table[k]] for k in at]
    else:
        runs = [fe.map_table(n)]
        assert sum(1 for _, exp in runs[0] if exp[0] & 0x40) >= 2
    for table in runs:
        got = ab_ctx.check_map_uniform([ub for ub, _ in table])
        assert "k_h2c_clear" in _clear_names(ab_ctx) and "k_slp_h2c" not in _clear_names(ab_ctx)
        monkeypatch.setenv("LSG_FP2_LANES", "0")
        old = ab_ctx.check_map_uniform([ub for ub, _ in table])
        assert "k_h2c_clear_pair" in _clear_names(ab_ctx) and "k_h2c_clear" not in _clear_names(ab_ctx)
        monkeypatch.delenv("LSG_FP2_LANES")
        assert got == old
        assert got == [exp for _, exp in table]


def test_h2c_clear_kernel_on_the_golden_messages(ab_ctx, monkeypatch):
    monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    gold = json.load(open(os.path.join(GOLDEN, "hash_to_g2.json")))
    by_len = {}
    for c in gold["cases"]:
        by_len.setdefault(len(c["msg"]), []).append(c)
    extra = [bd.msg("fp2-lanes", i) for i in range(33)]
    runs = [([bytes.fromhex(c["msg"]) for c in cs], [bytes.fromhex(c["out"]) for c in cs]) for cs in by_len.values()]
    runs.append((extra, [g2_serialize(h2c.hash_to_g2(m)) for m in extra]))
    for msgs, want in runs:
        got = ab_ctx.hash_to_g2(msgs)
        assert "k_h2c_clear" in _clear_names(ab_ctx) and "k_slp_h2c" not in _clear_names(ab_ctx)
        monkeypatch.setenv("LSG_FP2_LANES", "0")
        old = ab_ctx.hash_to_g2(msgs)
        assert "k_h2c_clear_pair" in _clear_names(ab_ctx)
        monkeypatch.delenv("LSG_FP2_LANES")
        assert got == old == want
