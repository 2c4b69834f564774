"""The fixed-exponent powers with one Fp element per lane (k_fp_pow_lanes, lodestar_amd/csrc/
lsg_fp2_lanes.hpp lanes_pow_plan) on the device: the kernel alone through lsg_check_pow_lanes at
the edges of a wave and a block, against the pair form's pair_pow_plan (lsg_check_pow_pair) word
for word and the oracle's field; then the signature decode and the SSWU map as stage kernels
around it (the A/B library with LSG_POW_LANES_MIN=1, so that small inputs take that path) against
the single pair-form kernels (LSG_POW_LANES=0) byte for byte and against the oracle; then one
package of the kind smoke() uses on the stage path.  Every comparison is exact.
Every test here needs an MI355X."""
import ctypes
import hashlib
import itertools
import json
import os

import pytest

from oracle import hash_to_curve as h2c
from oracle.curves import g2_serialize
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import field_edges as fe
from tests import sqr_patterns as sp

pytestmark = pytest.mark.gpu
P, RINV = sp.P, sp.RINV
R = 1 << 406
HI, LO = (1 << 29) + 8, -8  # the closed range of a carried limb
EXPONENTS = (P - 2, (P + 1) // 4, (P - 3) // 4)  # plan ids 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def names(c):
    return [nm for nm, _ in c.last_kernel_times()]


def _elements(n):
    """n elements: the limb extremes in the first and the last lane of the first two waves
    (elements 0, 63, 64, 127 where n reaches them), 0, 1, p - 1 (Montgomery form) in lazy
    representations, and the seeded patterns elsewhere"""
    ext = [sp.clamp([lo] * 13 + [top]) for lo, top in itertools.product((HI, LO), (sp.TOP_MAX, -sp.TOP_MAX))]
    pats = sp.fp_items()
    es = list(fe.E_VECTORS.values())
    special = [fe.rep(x * R % P, es[k % len(es)]) for k, x in enumerate((0, 1, P - 1, 0, P - 1, 1))]
    out = [special[i % 6] if i % 5 == 2 else pats[(7 * i + 3) % len(pats)] for i in range(n)]
    for at, e in zip((0, 63, 64, 127), ext):
        if at < n:
            out[at] = e
    if n >= 1:
        out[n - 1] = ext[(n + 1) % 4]  # the last live lane
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_power_kernel_against_the_pair_form_and_the_oracle(ctx, n):
    elems = _elements(n)
    w = [x for e in elems for x in sp.pair_words(e)]
    for pid, e in enumerate(EXPONENTS):
        got = ctx.check_pow(pid, w)
        assert names(ctx) == ["k_fp_pow_lanes"]
        old = ctx.check_pow(pid, w, lanes=False)
        assert names(ctx) == ["k_check_pow_pair"]
        assert got == old, (n, pid, [i for i in range(n) if got[14 * i:14 * i + 14] != old[14 * i:14 * i + 14]][:4])
        for i, a in enumerate(elems):
            r = sp.from_pair_words(got[14 * i:14 * i + 14])
            assert sp.value(r) * RINV % P == pow(sp.value(a) * RINV % P, e, P), (n, pid, i)
            assert all(0 <= v < (1 << 29) for v in r[:13]), (n, pid, i)


def _oracle_decode(s):
    """the C oracle's decode of a 96-byte encoding: (code, 192-byte point)"""
    L = co.lib()
    L.cpu_sig_decode.restype = ctypes.c_int
    L.cpu_sig_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    want = ctypes.create_string_buffer(192)
    return L.cpu_sig_decode(s, len(s), want), want.raw


def _decode_cases():
    """(encoding, expected code, expected 192-byte point) lists for the 96-byte and the 192-byte
    form: the golden decode cases (recorded from the oracle: codes 0, 1, 2, 3) and the encodings
    of the point at infinity, well-formed and not"""
    gold = json.load(open(os.path.join(GOLDEN, "sig_decode.json")))["cases"]
    cases = [(bytes.fromhex(c["sig"]), c["err"], bytes.fromhex(c["point"]) if c["err"] == 0 else None) for c in gold]
    c96 = [c for c in cases if len(c[0]) == 96]
    c192 = [c for c in cases if len(c[0]) == 192]
    assert {e for _, e, _ in c96} == {0, 1, 2, 3} and c192
    inf = bytes([0x40]) + bytes(191)
    c96.append((bytes([0xc0]) + bytes(95), 0, inf))
    c96.append((bytes([0xc0]) + bytes(94) + b"\1", 1, None))
    c192.append((inf, 0, inf))
    c192.append((bytes([0x40]) + bytes(190) + b"\1", 1, None))
    return c96, c192


@pytest.mark.parametrize("n", [1, 33, 65, 129])
def test_sig_decode_stage_kernels_against_single_kernel_and_oracle(ab_ctx, monkeypatch, n):
    c96, c192 = _decode_cases()
    wrong = [(bytes(95), 10, None), (bytes(97), 10, None)]  # LSG_BLST_INVALID_SIZE
    if n == 1:
        first = {}
        for c in c96:
            first.setdefault(c[1], c)
        batches = [[c] for c in list(first.values()) + c96[-2:] + [c192[0]] + c192[-2:] + wrong]
    else:  # every kind next to every other, rotated so each reaches the first and the last pair of a wave
        batches = [[c96[(i + 5 * r) % len(c96)] for i in range(n)] for r in range(3)]
        batches.append([c192[i % len(c192)] for i in range(n)])
        batches.append([wrong[0]] * n)  # every item in error before the powers
    seen = set()
    for batch in batches:
        sigs = [s for s, _, _ in batch]
        monkeypatch.setenv("LSG_POW_LANES_MIN", "1")
        got = ab_ctx.sig_decode(sigs)
        assert "k_fp_pow_lanes" in names(ab_ctx) and "k_sig_decode" in names(ab_ctx)
        monkeypatch.setenv("LSG_POW_LANES", "0")
        old = ab_ctx.sig_decode(sigs)
        assert "k_fp_pow_lanes" not in names(ab_ctx) and "k_sig_decode" in names(ab_ctx)
        monkeypatch.delenv("LSG_POW_LANES")
        assert got == old
        for k, ((s, werr, want), (pt, err)) in enumerate(zip(batch, got)):
            assert err == werr, (n, k, err, werr)
            if werr == 0:
                assert pt == want, (n, k)
            if len(s) == 96:
                assert _oracle_decode(s)[0] == werr, (n, k)  # the C oracle agrees with the record
            seen.add(err)
    assert {0, 1, 2, 3, 10} <= seen


@pytest.mark.parametrize("n", [1, 33, 130])
def test_map_stage_kernels_on_the_map_edges(ab_ctx, monkeypatch, n):
    """lsg_check_map_uniform: u = 0, the exceptional tv1 = 0 row, u1 = +-u0 among seeded inputs"""
    if n == 1:
        table = fe.map_table(33)
        runs = [[table[k]] for k in (0, 8, 11, 16, 32)]
    else:
        runs = [fe.map_table(n)]
    for table in runs:
        ubs = [ub for ub, _ in table]
        monkeypatch.setenv("LSG_POW_LANES_MIN", "1")
        got = ab_ctx.check_map_uniform(ubs)
        assert "k_fp_pow_lanes" in names(ab_ctx) and "k_h2c_map" in names(ab_ctx)
        monkeypatch.setenv("LSG_POW_LANES", "0")
        old = ab_ctx.check_map_uniform(ubs)
        assert "k_fp_pow_lanes" not in names(ab_ctx) and "k_h2c_map" in names(ab_ctx)
        monkeypatch.delenv("LSG_POW_LANES")
        assert got == old
        assert got == [exp for _, exp in table]


def test_map_stage_kernels_on_the_golden_messages(ab_ctx, monkeypatch):
    gold = json.load(open(os.path.join(GOLDEN, "hash_to_g2.json")))
    by_len = {}
    for c in gold["cases"]:
        by_len.setdefault(len(c["msg"]), []).append(c)
    extra = [bd.msg("pow-lanes", i) for i in range(33)]
    runs = [([bytes.fromhex(c["msg"]) for c in cs], [bytes.fromhex(c["out"]) for c in cs]) for cs in by_len.values()]
    runs.append((extra, [g2_serialize(h2c.hash_to_g2(m)) for m in extra]))
    for msgs, want in runs:
        monkeypatch.setenv("LSG_POW_LANES_MIN", "1")
        got = ab_ctx.hash_to_g2(msgs)
        assert "k_fp_pow_lanes" in names(ab_ctx)
        monkeypatch.setenv("LSG_POW_LANES", "0")
        old = ab_ctx.hash_to_g2(msgs)
        assert "k_fp_pow_lanes" not in names(ab_ctx)
        monkeypatch.delenv("LSG_POW_LANES")
        assert got == old == want


def test_package_on_the_stage_path(ab_ctx, monkeypatch):
    """the 296-job package of smoke(): 292 single-set batchable jobs, 4 two-set non-batchable
    jobs, one wrong-message set; verdicts and counters against the C oracle's worker rules"""
    from oracle.interop import interop_secret_key
    monkeypatch.setenv("LSG_POW_LANES_MIN", "1")
    n = 300
    sks = [interop_secret_key(i) for i in range(64)]
    pks = ab_ctx.sk_to_pk(sks)
    msgs = [hashlib.sha256(b"lodestar-mi355x" + b"pow-lanes-jobs" + i.to_bytes(8, "little")).digest() for i in range(n)]
    sigs = ab_ctx.sign([sks[i % 64] for i in range(n)], msgs)
    flat = [([pks[i % 64]], msgs[i], sigs[i]) for i in range(n)]
    flat[137] = bd.corrupt_wrong_message(flat[137])
    jobs = [([flat[i]], 1) for i in range(292)] + [(flat[292 + 2 * k:294 + 2 * k], 0) for k in range(4)]
    per = co.verify_each([p[0] for p, _, _ in flat], [m for _, m, _ in flat], [s for _, _, s in flat])
    assert per.count(0) == 1 and per[137] == 0
    jsets = [[i] for i in range(292)] + [[292 + 2 * k, 293 + 2 * k] for k in range(4)]
    exp, retries, success = co.expected_jobs(jsets, [True] * 292 + [False] * 4, per)
    got, stats = ab_ctx.verify_jobs(jobs)
    assert "k_fp_pow_lanes" in names(ab_ctx)
    assert [tuple(g) for g in got] == [tuple(e) for e in exp]
    assert (stats["batch_retries"], stats["batch_sigs_success"]) == (retries, success)
