"""The case tables of tests/field_edges.py through the host (x86) build of the pair backend
(tests/native/hostcheck.hip with LSG_PAIR_G = 1: all 14 limbs in one lane).  Proves without a
GPU that the tables and their expectations are right and pins the one-lane form of every
function; tests/test_gpu_field_edges.py runs the same tables through the device hooks, where
the lane pair's cross-lane moves come in.  Every comparison is exact."""
import ctypes

import pytest

from oracle.fields import P, f2_sqr
from tests import field_edges as fe
from tests import hostcheck_lib


@pytest.fixture(scope="module")
def hc():
    h = ctypes.CDLL(hostcheck_lib.build("pair"))  # a failed compile is an error, never a skip
    h.hc_canon.restype = ctypes.c_uint32
    h.hc_fp2_roots.restype = ctypes.c_uint32
    return h


def i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def canon(hc, limbs):
    """(pair_canon limbs, fp_canonical limbs, its 48 bytes, flags, the raw value's 48 bytes) of
    one raw element"""
    a, b = (ctypes.c_int32 * 14)(), (ctypes.c_int32 * 14)()
    by, raw = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48)
    f = hc.hc_canon(i32(limbs), a, b, by, raw)
    return list(a), list(b), by.raw, f, raw.raw


def roots(hc, a0, a1):
    """(root, fp_inv(a0), divstep inverse, flags) of raw limb vectors a0, a1; values as integers"""
    out = (ctypes.c_int32 * 56)()
    f = hc.hc_fp2_roots(i32(list(a0) + list(a1)), out)
    v = [fe.value(out[14 * k:14 * k + 14]) for k in range(4)]
    return (v[0], v[1]), v[2], v[3], f


def mont(x):
    return fe.norm_limbs(x * fe.R % P)


def test_rep_is_exact_and_in_range():
    # zero with a carry that ripples from limb 0 through every limb into the top one
    z = fe.rep(0, fe.E_VECTORS["all+8"])
    assert z == [1 << 29] + [(1 << 29) - 1] * 12 + [-1]
    for v in (0, 1, -1, P, -P, 4095 * P + 1, (1 << 203) - 1):
        for e in fe.E_VECTORS.values():
            assert fe.value(fe.rep(v, e)) == v


def test_pair_canon_and_is_zero(hc):
    for v, is_zero in fe.canon_values():
        for name, e in fe.E_VECTORS.items():
            c, _, _, f, _ = canon(hc, fe.rep(v, e))
            assert c == fe.norm_limbs(v % P), (v, name)
            assert bool(f & 1) == is_zero, (v, name)


def test_canonical_gt_half_parity(hc):
    for v in fe.canonical_values():
        m = v % P
        for name, e in fe.E_VECTORS.items():
            _, c, by, f, _ = canon(hc, fe.rep(v, e))
            assert c == fe.norm_limbs(m), (v, name)
            assert by == m.to_bytes(48, "big"), (v, name)
            assert bool(f & 4) == (m > fe.HALF_LO), (v, name)
            assert (f >> 3) & 1 == m & 1, (v, name)


def test_canon_lt_p(hc):
    for v in fe.lt_p_values():
        assert bool(canon(hc, fe.norm_limbs(v))[3] & 2) == (v < P), v


def test_bytes_in_and_out(hc):
    for v in fe.byte_values():
        out = (ctypes.c_int32 * 14)()
        hc.hc_from_be48(v.to_bytes(48, "big"), out)
        assert list(out) == fe.norm_limbs(v), v
        got = canon(hc, fe.norm_limbs(v))
        assert got[4] == v.to_bytes(48, "big"), v  # the raw form, flag bits 381..383 included
        if v < 2 * P:  # fp_canonical's domain: the bytes of the representative in [0, p)
            assert got[2] == (v % P).to_bytes(48, "big"), v


def test_fp2_sqrt_branches(hc):
    for a, exp in fe.root_expectations(fe.root_values()):
        r, _, _, f = roots(hc, mont(a[0]), mont(a[1]))
        assert bool(f & 1) == (exp is not None), a
        assert bool(f & 8) == (a == (0, 0)), a
        if exp is not None:
            got = (r[0] * fe.RINV % P, r[1] * fe.RINV % P)
            assert f2_sqr(got) == (a[0] % P, a[1] % P), a


def test_sgn0_and_lexi_largest(hc):
    for a in fe.sign_values():
        sgn, lexi = fe.sign_expect(a)
        forms = [(mont(a[0]), mont(a[1]))]
        forms += [(fe.rep(a[0] * fe.R % P, e), fe.rep(a[1] * fe.R % P, e)) for e in fe.E_VECTORS.values()]
        for a0, a1 in forms:
            f = roots(hc, a0, a1)[3]
            assert ((f >> 1) & 1, bool(f & 4)) == (sgn, lexi), (a, a0, a1)


def test_inversions(hc):
    for x in fe.inv_values():
        _, fermat, gcd, _ = roots(hc, fe.norm_limbs(x), [0] * 14)
        assert fe.inv_ok(x, fermat), x
        assert fe.inv_ok(x, gcd), x


@pytest.mark.parametrize("n,T", [(n, 16) for n in fe.LEVEL_SIZES + fe.BLOCK_SIZES[1:]] + [(8193, 2)])
def test_batch_inv_recurrences(hc, n, T):
    """the fold / unfold recurrences restated on the host (hc_binv), at the sizes of both
    device forms; the one-launch form's LDS heap exists on the device only"""
    for name, elems in fe.batch_cases(n, T, T):
        flat = [w for e in elems for w in e]
        out = (ctypes.c_int32 * (14 * n))()
        assert hc.hc_batch_inv(i32(flat), n, T, out) == 0
        for k, e in enumerate(elems):
            assert fe.inv_ok(fe.value(e), fe.value(out[14 * k:14 * k + 14])), (name, n, k)


@pytest.mark.parametrize("n", fe.MAP_SIZES)
def test_map_from_uniform_bytes(hc, n):
    table = fe.map_table(n)
    assert sum(1 for _, exp in table if exp[0] & 0x40) >= 2  # the identity is among the cases
    for k, (ub, exp) in enumerate(table):
        out = ctypes.create_string_buffer(192)
        hc.hc_map_uniform(ub, out)
        assert out.raw == exp, (n, k)
