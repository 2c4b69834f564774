"""The case tables of tests/field_edges.py through the device hooks lsg_check_canon,
lsg_check_fp2_roots, lsg_check_batch_inv and lsg_check_map_uniform (include/lodestar_bls.h): the
lane-pair form of the canonical forms, predicates, byte conversions, Fp2 roots and signs,
inversions and the SSWU / infinity edge cases, whose cross-lane moves (pup, pswap, pbcast,
pair_gather) the one-lane host build of tests/test_field_edges_host.py never executes.  Every
comparison is an exact integer or byte comparison against Python integers and oracle/."""
import pytest

from oracle.fields import P, f2_sqr
from tests import field_edges as fe
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def words(elems):
    return [w for e in elems for w in sp.pair_words(e)]


def limbs_at(out, off):
    return sp.from_pair_words(out[off:off + 14])


def be48_at(out, off):
    return b"".join(w.to_bytes(4, "little") for w in out[off:off + 12])


def mont(x):
    return fe.norm_limbs(x * fe.R % P)


def test_pair_canon_and_is_zero(ctx):
    cases = [(v, z, name, fe.rep(v, e)) for v, z in fe.canon_values() for name, e in fe.E_VECTORS.items()]
    out, _ = ctx.check_canon(words(c[3] for c in cases))
    for i, (v, is_zero, name, _) in enumerate(cases):
        assert limbs_at(out, 54 * i) == fe.norm_limbs(v % P), (v, name)
        assert bool(out[54 * i + 40] & 1) == is_zero, (v, name)
        assert out[54 * i + 41] == 0


def test_canonical_gt_half_parity(ctx):
    cases = [(v, name, fe.rep(v, e)) for v in fe.canonical_values() for name, e in fe.E_VECTORS.items()]
    out, _ = ctx.check_canon(words(c[2] for c in cases))
    for i, (v, name, _) in enumerate(cases):
        m, f = v % P, out[54 * i + 40]
        assert limbs_at(out, 54 * i + 14) == fe.norm_limbs(m), (v, name)
        assert be48_at(out, 54 * i + 28) == m.to_bytes(48, "big"), (v, name)
        assert bool(f & 4) == (m > fe.HALF_LO), (v, name)
        assert (f >> 3) & 1 == m & 1, (v, name)
        assert bool(f & 1) == (m == 0), (v, name)


def test_canon_lt_p(ctx):
    vs = fe.lt_p_values()
    out, _ = ctx.check_canon(words(fe.norm_limbs(v) for v in vs))
    for i, v in enumerate(vs):
        assert bool(out[54 * i + 40] & 2) == (v < P), v


def test_bytes_in_and_out(ctx):
    vs = fe.byte_values()
    out, limbs = ctx.check_canon(words(fe.norm_limbs(v) for v in vs), [v.to_bytes(48, "big") for v in vs])
    for i, v in enumerate(vs):
        assert limbs_at(limbs, 14 * i) == fe.norm_limbs(v), v
        # the raw form, flag bits 381..383 included, as the compressed encodings are written
        assert be48_at(out, 54 * i + 42) == v.to_bytes(48, "big"), v
        if v < 2 * P:  # fp_canonical's domain: the bytes of the representative in [0, p)
            assert be48_at(out, 54 * i + 28) == (v % P).to_bytes(48, "big"), v


def test_fp2_sqrt_branches(ctx):
    exp = fe.root_expectations(fe.root_values())
    out = ctx.check_fp2_roots(words(m for a, _ in exp for m in (mont(a[0]), mont(a[1]))))
    for i, (a, root) in enumerate(exp):
        f = out[58 * i + 56]
        assert bool(f & 1) == (root is not None), a
        assert bool(f & 8) == (a == (0, 0)), a
        assert out[58 * i + 57] == 0
        if root is not None:
            got = tuple(fe.value(limbs_at(out, 58 * i + 14 * k)) * fe.RINV % P for k in range(2))
            assert f2_sqr(got) == (a[0] % P, a[1] % P), a


def test_sgn0_and_lexi_largest(ctx):
    cases = []
    for a in fe.sign_values():
        cases.append((a, "normalised", mont(a[0]), mont(a[1])))
        cases += [(a, name, fe.rep(a[0] * fe.R % P, e), fe.rep(a[1] * fe.R % P, e)) for name, e in fe.E_VECTORS.items()]
    out = ctx.check_fp2_roots(words(m for c in cases for m in c[2:]))
    for i, (a, name, _, _) in enumerate(cases):
        f = out[58 * i + 56]
        assert ((f >> 1) & 1, bool(f & 4)) == fe.sign_expect(a), (a, name)
        assert bool(f & 8) == (a == (0, 0)), (a, name)


def test_inversions(ctx):
    vs = fe.inv_values()
    out = ctx.check_fp2_roots(words(m for x in vs for m in (fe.norm_limbs(x), [0] * 14)))
    for i, x in enumerate(vs):
        assert fe.inv_ok(x, fe.value(limbs_at(out, 58 * i + 28))), ("fp_inv", x)
        assert fe.inv_ok(x, fe.value(limbs_at(out, 58 * i + 42))), ("pair_inv_gcd", x)


def test_hooks_reject_null_and_oversized(ctx):
    from lodestar_amd._native import LSG_ERR_INVALID_ARG
    lib, h, buf, big = ctx.lib, ctx.h, bytes(256), 1 << 31
    for rc in (lib.lsg_check_canon(h, None, 1, None, 0, buf, None), lib.lsg_check_canon(h, buf, 1, None, 0, None, None),
               lib.lsg_check_canon(h, None, 0, buf, 1, None, None), lib.lsg_check_canon(h, buf, big, None, 0, buf, None),
               lib.lsg_check_canon(h, None, 0, buf, big, None, buf), lib.lsg_check_canon(None, buf, 1, None, 0, buf, None)):
        assert rc == LSG_ERR_INVALID_ARG
    for fn in (lib.lsg_check_fp2_roots, lib.lsg_check_batch_inv, lib.lsg_check_map_uniform):
        assert [fn(h, None, 1, buf), fn(h, buf, 1, None), fn(h, buf, big, buf), fn(None, buf, 1, buf)] == \
            [LSG_ERR_INVALID_ARG] * 4
        assert fn(h, None, 0, None) == 0


def _batch_inv(c, n, chunk, block):
    for name, elems in fe.batch_cases(n, chunk, block):
        out = c.check_batch_inv(words(elems))
        for k, e in enumerate(elems):
            assert fe.inv_ok(fe.value(e), fe.value(limbs_at(out, 14 * k))), (name, n, k)
    return [nm for nm, _ in c.last_kernel_times()]


@pytest.mark.parametrize("n", fe.BLOCK_SIZES)
def test_batch_inv_one_launch(ctx, n):
    T = fe.block_chunk(n)
    assert (T == 2) == (n == 8193)
    assert _batch_inv(ctx, n, T, 128 * T) == ["binv_check"]  # k_binv_block


@pytest.mark.parametrize("n", fe.LEVEL_SIZES)
def test_batch_inv_levels(ab_ctx, monkeypatch, n):
    monkeypatch.setenv("LSG_BINV_BLOCK", "0")
    levels = 0
    m = n
    while m > 1:
        m = (m + 15) // 16
        levels += 1
    # k_binv_fold per level, k_binv_root, k_binv_unfold per level
    assert _batch_inv(ab_ctx, n, 16, 16) == ["binv_check"] * (2 * levels + 1)


def _map(c, n):
    table = fe.map_table(n)
    assert sum(1 for _, exp in table if exp[0] & 0x40) >= 2  # the identity is among the cases
    got = c.check_map_uniform([ub for ub, _ in table])
    for k, ((_, exp), o) in enumerate(zip(table, got)):
        assert o == exp, (n, k)
    return [nm for nm, _ in c.last_kernel_times()]


@pytest.mark.parametrize("n", fe.MAP_SIZES)
def test_map_uniform_program_path(ctx, n):
    names = _map(ctx, n)
    assert names == ["k_h2c_prep", "binv_sswu", "k_h2c_map", "k_slp_h2c", "k_g2a_to_bytes"]


@pytest.mark.parametrize("n", fe.MAP_SIZES)
def test_map_uniform_kernel_path(ab_ctx, monkeypatch, n):
    monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    names = _map(ab_ctx, n)
    assert names == ["k_h2c_prep", "binv_sswu", "k_h2c_map", "k_h2c_clear", "binv_hash", "k_h2c_affine",
                     "k_g2a_to_bytes"]


@pytest.mark.parametrize("kernels", [False, True])
@pytest.mark.parametrize("n", fe.MAP_SIZES)
def test_map_uniform_level_inversions(ab_ctx, monkeypatch, n, kernels):
    """the fold / root / unfold inversions under the map, with the program path and (kernels)
    with k_h2c_clear / k_h2c_affine, whose binv_hash then inverts the identity's zero norm"""
    monkeypatch.setenv("LSG_BINV_BLOCK", "0")
    if kernels:
        monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    names = _map(ab_ctx, n)
    assert names.count("binv_sswu") >= 3
    if kernels:
        assert names.count("binv_hash") >= 3 and "k_h2c_clear" in names and "k_h2c_affine" in names
    else:
        assert "k_slp_h2c" in names
