"""Sets spanning several committees on the GPU (LSG_PK_BITS_MULTI, k_pk_agg_bits_multi: a
committee list + one bitfield over the concatenation of the listed committees, the shape of an
EIP-7549 aggregate), against the same sets given by table index, the Python oracle's
PublicKey.aggregate and tests/cpu_oracle.py's worker.ts rules.  Every comparison is exact (bytes
and integers).  Every test here needs an MI355X.

The table is the one of tests/test_gpu_committees.py: 600 rows, the keys of secret keys 1..64
repeated, the infinity key at row 100, row 200 left unset, P / -P at rows 300 / 301.  The
committees: one per length (ids 10..), the special ones (ids 900..), the verdict package's
(ids 2000..).
"""
import ctypes
import hashlib
import random

import pytest

from oracle.fields import R
from tests import cpu_oracle as co
from tests import msgobjects as mo
from tests.test_gpu_committees import (INF96, ROW_NEG_P, ROW_P, ROW_UNSET, ROWS, Table, bits_of, pack, usable_rows)

pytestmark = pytest.mark.gpu
B, V = 1, 4  # LSG_JOB_BATCHABLE, LSG_JOB_VALIDATE_KEYS
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 450]
PART_COUNTS = [1, 2, 3, 64]
ERR_INVALID_ARG, ERR_EMPTY_AGGREGATE, ERR_BAD_INDEX, ERR_BAD_COMMITTEE = 1, 101, 102, 103
ROW_INF = 100
DUP = [5, 5, 5, 9, 9, ROW_P, 5]
WITH_INF = [ROW_INF, 1, 2, ROW_INF, 3]
P_NEG_P = [ROW_P, ROW_NEG_P]
CANCEL_BUT_ONE = [ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, 7]
NEG_SUM = [ROW_P, ROW_NEG_P, ROW_NEG_P, ROW_P, ROW_NEG_P]
SUM_INF = [ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P]
SPECIAL = {"dup": DUP, "with_inf": WITH_INF, "p_neg_p": P_NEG_P, "cancel_but_one": CANCEL_BUT_ONE, "neg_sum": NEG_SUM,
           "sum_inf": SUM_INF}
FIRST_LEN_ID, FIRST_SPECIAL_ID, FIRST_VERDICT_ID = 10, 900, 2000
SID = {name: FIRST_SPECIAL_ID + k for k, name in enumerate(SPECIAL)}
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job")


def length_committees():
    rng = random.Random(1811)
    return [usable_rows(rng, n) for n in LENGTHS]


def register(ctx):
    lens = length_committees()
    assert ctx.committees_set(FIRST_LEN_ID, lens) == [0] * len(lens)
    assert ctx.committees_set(FIRST_SPECIAL_ID, list(SPECIAL.values())) == [0] * len(SPECIAL)
    return lens


@pytest.fixture(scope="module")
def table():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    try:
        return Table(c)
    finally:
        c.close()


@pytest.fixture(scope="module")
def ctx(table):
    from lodestar_amd._native import Context
    c = Context(0)
    table.load(c)
    register(c)
    yield c
    c.close()


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def pattern(name, n, rng):
    if name == "empty":
        return [0] * n
    if name == "full":
        return [1] * n
    if name in ("one_absent", "one_present"):
        b = [1 if name == "one_absent" else 0] * n
        b[rng.randrange(n)] ^= 1
        return b
    if name == "alternating":
        return [k & 1 for k in range(n)]
    q = {"random_1": 0.01, "random_50": 0.5, "random_99": 0.99}[name]
    return [1 if rng.random() < q else 0 for _ in range(n)]


PATTERNS = ["empty", "full", "one_absent", "one_present", "alternating", "random_1", "random_50", "random_99"]


class MultiCase:
    """one multi set: (committee id, its rows, its bits) per part"""

    def __init__(self, parts):
        self.parts = parts
        self.ids = [cid for cid, _, _ in parts]
        self.bits = [b for _, _, pb in parts for b in pb]
        self.rows = [r for _, rows, pb in parts for r in bits_of(rows, pb)]

    def multi(self, garbage=None):
        from lodestar_amd._native import PkBitsMulti
        raw = pack(self.bits, garbage)
        if garbage is not None:
            raw += bytes([garbage.randrange(256)])  # noise past n_pks
        return PkBitsMulti(self.ids, raw, len(self.bits))

    def index(self):
        from lodestar_amd._native import PkIndices
        return PkIndices(self.rows)


# ---- 1. aggregates
def aggregate_cases():
    rng = random.Random(15)
    lens = length_committees()
    cases = []
    for k in PART_COUNTS:
        firsts = range(len(LENGTHS)) if k < 64 else (0, 6, 11)  # (64 parts: three first parts)
        for first in firsts:
            for pi, name in enumerate(PATTERNS if k < 64 else PATTERNS[first % 3::3]):
                cs = [first] + [rng.randrange(len(LENGTHS) - (1 if k == 64 else 0)) for _ in range(k - 1)]
                nm = [name] + [PATTERNS[(pi + e) % len(PATTERNS)] for e in range(1, k)]
                cases.append(MultiCase([(FIRST_LEN_ID + c, lens[c], pattern(n_, LENGTHS[c], rng)) for n_, c in zip(nm, cs)]))
    # every pattern on all parts at once; 64 parts all full: 64 stored sums and no member
    for name in PATTERNS:
        cs = [rng.randrange(len(LENGTHS) - 1) for _ in range(3)]
        cases.append(MultiCase([(FIRST_LEN_ID + c, lens[c], pattern(name, LENGTHS[c], rng)) for c in cs]))
    cases.append(MultiCase([(FIRST_LEN_ID + c % 11, lens[c % 11], [1] * LENGTHS[c % 11]) for c in range(64)]))
    # one committee of 450 among short ones, repeated ids
    cases.append(MultiCase([(FIRST_LEN_ID + c, lens[c], pattern("random_99", LENGTHS[c], rng)) for c in (11, 3, 11, 3, 0)]))

    def special(*parts):
        return MultiCase([(SID[name], SPECIAL[name], list(bits)) for name, bits in parts])
    named = [
        special(("dup", [1] * 7), ("with_inf", [1] * 5)),
        special(("with_inf", [1, 0, 0, 1, 0]), ("dup", [1, 1, 0, 1, 0, 0, 1])),   # a part whose participants are infinity keys
        special(("p_neg_p", [1, 1]), ("dup", [1] * 7)),                            # complement part whose sum is infinity
        special(("cancel_but_one", [1, 1, 1, 1, 1, 1, 0]), ("p_neg_p", [1, 0])),   # complement: acc = -absentee, then + sum
        special(("neg_sum", [0, 1, 1, 1, 1]), ("neg_sum", [1, 1, 1, 1, 1])),       # complement: absentees == -sum
        special(("sum_inf", [0, 1, 1, 1, 1, 1]), ("dup", [0, 0, 0, 1, 0, 0, 0])),
        special(("p_neg_p", [1, 0]), ("p_neg_p", [0, 1])),                         # P, then -P: the total is infinity
        special(("p_neg_p", [1, 1])),                                              # ... as one complement part
        special(("sum_inf", [1] * 6), ("p_neg_p", [1, 1]), ("sum_inf", [1] * 6)),  # ... as three sums at infinity
        special(("neg_sum", [1] * 5), ("p_neg_p", [1, 0])),                        # sum -P, then +P: infinity
    ]
    return cases, named


def test_aggregates_match_index_sets_and_oracle(ctx, table):
    from lodestar_amd._native import PkBits
    rng = random.Random(51)
    cases, named = aggregate_cases()
    every = cases + named
    want = [table.aggregate(c.rows) for c in every]
    by_multi = ctx.aggregate_pubkeys_multi([c.multi(rng) for c in every])
    got = names(ctx)
    assert "k_pk_agg_bits_multi" in got and "g1_aggregate" not in got and "k_pk_agg_bits" not in got, got
    by_index = ctx.aggregate_pubkeys_multi([c.index() for c in every])
    got = names(ctx)
    assert "g1_aggregate" in got and "k_pk_agg_bits_multi" not in got, got
    bad = [(i, every[i].ids[:4], len(every[i].bits), sum(every[i].bits)) for i in range(len(every))
           if not (by_multi[i] == by_index[i] == want[i])]
    assert not bad, bad[:10]
    assert {w[1] for w in want} == {0, ERR_EMPTY_AGGREGATE}
    # the named totals at infinity, whatever the three agree on
    assert [w for w in want[-4:]] == [(INF96, 0)] * 4
    # a one-part multi set is the LSG_PK_BITS set, byte for byte
    ones = [c for c in cases if len(c.parts) == 1]
    assert len(ones) == len(LENGTHS) * len(PATTERNS)
    as_bits = ctx.aggregate_pubkeys_multi([PkBits(c.ids[0], pack(c.bits), len(c.bits)) for c in ones])
    assert as_bits == ctx.aggregate_pubkeys_multi([c.multi() for c in ones])
    # a call mixing the four forms: each set takes its own path
    c0 = named[0]
    mixed = ctx.aggregate_pubkeys_multi([c0.multi(), c0.index(), [table.enc[r] for r in c0.rows],
                                         PkBits(SID["dup"], pack([1] * 7), 7)])
    assert mixed == [table.aggregate(c0.rows)] * 3 + [table.aggregate(DUP)]
    got = names(ctx)
    assert "k_pk_agg_bits_multi" in got and "k_pk_agg_bits" in got and "g1_aggregate" in got, got
    # the single-list call does not know the form
    out, err = ctx.aggregate_pubkeys([bytes(12)] * 2)
    assert err == 10  # BLST_INVALID_SIZE, as for any unknown key length


# ---- 2. verdicts
def register_verdict_committees(ctx):
    rng = random.Random(1413)
    committees = [usable_rows(rng, n) for n in (3, 17, 33, 64, 65, 130, 450)]
    assert ctx.committees_set(FIRST_VERDICT_ID, committees) == [0] * len(committees)
    return committees


def verdict_package(ctx, table):
    """Jobs of 1-3 sets mixing byte, index, bits and multi sets, batchable and not; some forged;
    four sets share one message; some messages are AttestationData objects + domain.  Returns
    (jobs with bits / multi sets, the same with index sets, per-set oracle outcomes)."""
    from lodestar_amd._native import MsgObject, PkBits, PkBitsMulti, PkIndices
    rng = random.Random(1414)
    committees = register_verdict_committees(ctx)
    domain = rng.randbytes(32)
    shared = hashlib.sha256(b"lodestar-mi355x" + b"multi-shared").digest()
    n_sets = 40
    sets = []  # [form, committee indices, flat rows, flat bits, msg as given, signing root, sig]
    for i in range(n_sets):
        form = ("multi", "index", "bytes", "bits", "multi")[i % 5]
        if form == "bits":
            ks = [i % len(committees)]
        elif i == 25:
            ks = [2, 2, 0, 2]  # repeated ids, not ascending
        else:
            ks = [rng.randrange(len(committees)) for _ in range(1 + i % 4)]
        q = [0.99, 0.9, 0.5][i % 3]
        bits = [1 if rng.random() < q else 0 for k in ks for _ in committees[k]]
        bits[rng.randrange(len(bits))] = 1
        if i in (5, 6, 10, 15):
            msg = root = shared
        elif i % 8 == 2:
            data = rng.randbytes(128)  # AttestationData bytes
            msg, root = MsgObject(data, domain), mo.signing_root(data, domain)
        else:
            msg = root = hashlib.sha256(b"lodestar-mi355x" + b"multi" + i.to_bytes(8, "little")).digest()
        sets.append([form, ks, [r for k in ks for r in committees[k]], bits, msg, root, None])
    assert [sets[i][0] for i in (4, 14, 15, 20, 34)] == ["multi"] * 5
    sks = [sum(table.sk[r] for r in bits_of(st[2], st[3])) % R for st in sets]
    assert all(sks)
    for st, sig in zip(sets, ctx.sign(sks, [st[5] for st in sets])):
        st[6] = sig
    forged = {}
    for i, kind in ((4, "wrong_bit"), (14, "absentee"), (15, "wrong_bit"), (20, "signature"), (27, "absentee")):
        _, _, rows, bits, _, _, _ = sets[i]
        if kind == "signature":
            sets[i][6] = sets[i + 1][6]  # decodes, does not verify
        else:
            flip = [j for j, b in enumerate(bits) if b == (1 if kind == "wrong_bit" else 0) and table.sk[rows[j]] != 0]
            if not flip:  # (nothing absent: clear a bit instead)
                flip = [j for j, b in enumerate(bits) if b and table.sk[rows[j]] != 0]
            bits[flip[len(flip) // 2]] ^= 1
        forged[i] = kind
    as_multi, as_index, agg = [], [], []
    for form, ks, rows, bits, msg, _root, sig in sets:
        part = bits_of(rows, bits)
        agg.append(table.aggregate(part)[0])
        ids = [FIRST_VERDICT_ID + k for k in ks]
        alt = {"multi": PkBitsMulti(ids, pack(bits), len(bits)), "bits": PkBits(ids[0], pack(bits), len(bits)),
               "index": PkIndices(part), "bytes": [table.enc[r] for r in part]}
        as_multi.append((alt[form], msg, sig))
        as_index.append((alt["index" if form in ("bits", "multi") else form], msg, sig))
    per_set = co.verify_each(agg, [s[5] for s in sets], [s[6] for s in sets])
    assert [i for i, v in enumerate(per_set) if v != 1] == sorted(forged), (per_set, forged)
    shape, pos = [], 0
    while pos < n_sets:
        cnt = min(1 + len(shape) % 3, n_sets - pos)
        shape.append((pos, cnt, B if len(shape) % 5 != 3 else 0))
        pos += cnt

    def jobs(flat):
        return [(flat[p:p + c], f) for p, c, f in shape]
    return jobs(as_multi), jobs(as_index), per_set


def expected(jobs, per_set):
    jsets, pos = [], 0
    for sets, _ in jobs:
        jsets.append(list(range(pos, pos + len(sets))))
        pos += len(sets)
    return co.expected_jobs(jsets, [bool(f & B) for _, f in jobs], per_set)


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


@pytest.fixture(scope="module")
def package(ctx, table):
    jm, ji, per_set = verdict_package(ctx, table)
    exp, retries, success = expected(jm, per_set)
    assert {e[0] for e in exp} == {0, 1}
    return {"multi": jm, "index": ji, "exp": exp, "retries": retries, "success": success}


def check(got, stats, package, counters=True):
    assert norm(got) == package["exp"]
    assert stats["key_error"] == 0
    if counters:
        assert (stats["batch_retries"], stats["batch_sigs_success"]) == (package["retries"], package["success"]), stats


def test_verdicts_of_a_mixed_package(ctx, package):
    from lodestar_amd._native import PkBitsMulti
    got_m, stats_m = ctx.verify_jobs(package["multi"], seed=3)
    got = names(ctx)
    # multi, bits and ordinary sets, each its own way; the objects' roots on the device
    assert "k_pk_agg_bits_multi" in got and "k_pk_agg_bits" in got and "g1_aggregate" in got and "k_msg_roots" in got, got
    check(got_m, stats_m, package)
    got_i, stats_i = ctx.verify_jobs(package["index"], seed=3)
    assert "k_pk_agg_bits_multi" not in names(ctx)
    assert got_m == got_i
    assert [stats_m[k] for k in COUNTERS] == [stats_i[k] for k in COUNTERS]
    # one job of multi sets through maybeBatch (lsg_verify_sets), valid and forged
    flat = [s for sets, _ in package["multi"] for s in sets]
    assert all(isinstance(flat[i][0], PkBitsMulti) for i in (0, 4, 5, 9, 10))
    assert ctx.verify_sets([flat[0], flat[5], flat[9], flat[10]]) == (1, 0)
    assert ctx.verify_sets([flat[0], flat[4], flat[9]]) == (0, 0)
    # lsg_batch_partial: the shard of multi sets alone
    only = [s for s in flat if isinstance(s[0], PkBitsMulti)]
    good = [s for s in only if s not in (flat[4], flat[14], flat[15], flat[20])]
    part, errs, anyerr = ctx.batch_partial(good, seed=8)
    assert not anyerr and errs == [0] * len(good) and ctx.final_verify([part])
    part_i, _, _ = ctx.batch_partial([fi for fm, fi in zip(flat, [s for sets, _ in package["index"] for s in sets])
                                      if fm in good], seed=8)
    assert part == part_i  # the exported partial is the index form's
    part, errs, anyerr = ctx.batch_partial(only, seed=8)
    assert not anyerr and not ctx.final_verify([part])


def test_grouped_package_aggregates_match_the_index_form(ctx, package):
    n_sets = sum(len(s) for s, _ in package["multi"])
    groups = [i % 5 if i % 7 else 0xFFFFFFFF for i in range(n_sets)]
    got_m, stats_m, agg_m = ctx.verify_jobs_grouped(package["multi"], groups, 5, seed=13)
    assert "k_pk_agg_bits_multi" in names(ctx)
    got_i, stats_i, agg_i = ctx.verify_jobs_grouped(package["index"], groups, 5, seed=13)
    check(got_m, stats_m, package, counters=False)
    assert got_m == got_i and agg_m == agg_i and sum(n for _, n in agg_m) > 0
    assert [stats_m[k] for k in COUNTERS] == [stats_i[k] for k in COUNTERS]


# ---- 3. errors
def test_errors(table):
    from lodestar_amd._native import Context, LsgJobResult, PkBitsMulti, SetBuffer
    c = Context(0)
    try:
        table.load(c)
        good_rows, four, stale_rows = [1, 2, 3, 4, 5, 6, 7, 8, 9], [11, 12, 13, 14], [20, 21, 22, 23]
        errs = c.committees_set(0, [good_rows, [1, ROW_UNSET, 2], four, stale_rows, [30, 31]])
        assert errs == [0, ERR_BAD_INDEX, 0, 0, 0]
        msgs = [hashlib.sha256(b"lodestar-mi355x" + b"cm-multi-errors" + bytes([i])).digest() for i in range(4)]
        rows_of = {0: good_rows, 1: [1, ROW_UNSET, 2], 2: four, 3: stale_rows, 4: [30, 31], 77: good_rows}

        def signed(ids, bits, msg, n_bits=None):
            rows = [r for cid in ids for r in rows_of.get(cid, good_rows)]
            sk = sum(table.sk[r] for r in bits_of(rows, bits) if table.sk[r]) % R
            return (PkBitsMulti(ids, pack(bits), len(bits) if n_bits is None else n_bits), msg, c.sign([sk or 1], [msg])[0])
        ok = [signed([0, 2], [1] * 13, msgs[0]), signed([2, 0], [1, 0, 1, 1] + [1] * 8 + [0], msgs[1]),
              signed([3, 4, 3], [1] * 10, msgs[2])]

        def run(third, flags=B):
            return c.verify_jobs([([ok[0]], B), ([ok[1]], flags), ([third], B), ([ok[2]], 0)], seed=17)
        got, stats = run(ok[0])
        assert norm(got) == [(1, 0)] * 4 and stats["key_error"] == 0

        def rejected(bad):
            got, stats = run(bad)
            assert (stats["key_error"], stats["key_error_job"]) == (ERR_BAD_COMMITTEE, 2), stats
            assert norm(got) == [(2, ERR_BAD_COMMITTEE)] * 4
            assert c.aggregate_pubkeys_multi([bad[0], ok[0][0]])[0][1] == ERR_BAD_COMMITTEE
            part, errs, anyerr = c.batch_partial([ok[0], bad], seed=2)
            assert anyerr and errs == [0, ERR_BAD_COMMITTEE]
        for bad in (signed([0, 77], [1] * 18, msgs[3]),               # unknown id
                    signed([1 << 20, 0], [1] * 18, msgs[3], n_bits=9),
                    signed([0, 1], [1] * 12, msgs[3]),                 # left unset: names the unset row
                    signed([0, 2], [1] * 13, msgs[3], n_bits=14),      # length mismatch
                    signed([0, 2], [1] * 12, msgs[3]),
                    signed([0, 2, 2], [1] * 13, msgs[3]),
                    signed([], [1] * 9, msgs[3])):                     # k == 0 with n_pks > 0
            rejected(bad)
        # no participant: EMPTY_AGGREGATE_ARRAY for its job only, and the error of a bad id comes first
        for empty in ((PkBitsMulti([0, 2], bytes(2), 13), msgs[3], ok[0][2]),
                      (PkBitsMulti([0, 2], b"\x00\xe0\xff", 13), msgs[3], ok[0][2]),  # (bits past n_pks do not count)
                      (PkBitsMulti([], b"", 0), msgs[3], ok[0][2])):
            got, stats = run(empty)
            assert norm(got) == [(1, 0), (1, 0), (2, ERR_EMPTY_AGGREGATE), (1, 0)] and stats["key_error"] == 0
            assert c.aggregate_pubkeys_multi([empty[0]]) == [(INF96, ERR_EMPTY_AGGREGATE)]
        rejected((PkBitsMulti([0, 77], bytes(3), 18), msgs[3], ok[0][2]))
        # caller bugs: more than 64 committees, no blob -- LSG_ERR_INVALID_ARG, nothing staged,
        # and the next package on the same context verifies
        many = (PkBitsMulti([4] * 65, b"\xff" * 17, 130), msgs[3], ok[0][2])
        for call in (lambda: run(many), lambda: c.verify_sets([ok[0], many]), lambda: c.batch_partial([many]),
                     lambda: c.aggregate_pubkeys_multi([ok[0][0], many[0]]),
                     lambda: c.verify_jobs_grouped([([ok[0], many], B)], [0, 0], 1)):
            with pytest.raises(RuntimeError, match=r"failed \(1\)"):
                call()
            assert norm(run(ok[0])[0]) == [(1, 0)] * 4
        assert c.aggregate_pubkeys_multi([PkBitsMulti([4] * 64, b"\xff" * 16, 128)])[0][1] == 0  # 64 are fine
        null = SetBuffer([ok[0], ok[1]])
        null.arr[1].pks = None
        res = LsgJobResult()
        assert c.lib.lsg_verify_sets(c.h, null.arr, null.n, 5, ctypes.byref(res)) == ERR_INVALID_ARG
        out, err = ctypes.create_string_buffer(192), (ctypes.c_int32 * 2)()
        assert c.lib.lsg_aggregate_pubkeys_multi(c.h, null.arr, 2, out, err) == ERR_INVALID_ARG
        null.arr[1].n_pks = 0
        assert c.lib.lsg_aggregate_pubkeys_multi(c.h, null.arr, 2, out, err) == ERR_INVALID_ARG
        assert norm(run(ok[0])[0]) == [(1, 0)] * 4
        # LSG_JOB_VALIDATE_KEYS leaves multi sets alone
        plain = run(ok[0])
        flagged = run(ok[0], flags=B | V)
        assert flagged[0] == plain[0] and [flagged[1][k] for k in COUNTERS] == [plain[1][k] for k in COUNTERS]
        assert not [k for k in names(c) if "keyvalidate" in k]
        # a cleared id is unknown; a rewrite of any table row unsets every committee
        c.committees_clear(4, 1)
        got, stats = run(ok[0])
        assert (stats["key_error"], stats["key_error_job"]) == (ERR_BAD_COMMITTEE, 3) and norm(got) == [(2, ERR_BAD_COMMITTEE)] * 4
        assert c.committees_set(4, [[30, 31]]) == [0] and norm(run(ok[0])[0]) == [(1, 0)] * 4
        assert c.pubkey_table_set(ROWS, [table.enc[3]]) == [0]  # (an append leaves them set)
        assert norm(run(ok[0])[0]) == [(1, 0)] * 4
        assert c.pubkey_table_set(21, [table.enc[21]]) == [0]
        assert c.committee_count() == 0
        got, stats = run(ok[0])
        assert (stats["key_error"], stats["key_error_job"]) == (ERR_BAD_COMMITTEE, 0)
        assert c.committees_set(0, [good_rows]) == [0] and c.committees_set(2, [four, stale_rows, [30, 31]]) == [0] * 3
        assert norm(run(ok[0])[0]) == [(1, 0)] * 4
    finally:
        c.close()


# ---- 4. everywhere jobs go
def test_coalesced_packages(table, package):
    from lodestar_amd._native import Context
    c = Context(0)
    try:
        table.load(c)
        register_verdict_committees(c)
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        tickets = [c.submit_jobs(p, seed=29) for p in (package["multi"], package["index"], package["multi"])]
        assert all(t is not None and t[0] >> 8 & 255 == 4 for t in tickets)  # coalesced tickets
        res = [c.wait_jobs(t) for t in tickets]
        for got, stats in res:
            check(got, stats, package)
        assert res[0][0] == res[1][0] == res[2][0]
    finally:
        c.close()


def test_multi_device_duplicate_ids(table, package):
    from lodestar_amd._native import Context
    c = Context(devices=[0, 0, 0])
    try:
        assert c.device_count() == 3
        table.load(c)
        register_verdict_committees(c)
        got, stats = c.verify_jobs(package["multi"], seed=31)
        check(got, stats, package, counters=False)  # (chunks are formed per device)
        got_i, _ = c.verify_jobs(package["index"], seed=31)
        assert got == got_i
    finally:
        c.close()


def test_node_protocol(ctx, package):
    good = [(sets, f) for (sets, f), e in zip(package["multi"], package["exp"]) if e == (1, 0)]
    t = ctx.submit_jobs(good, seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and ctx.final_verify([part])
    got, _ = ctx.wait_jobs_node(t, 1)
    assert norm(got) == [(1, 0)] * len(good)
    for node_valid in (1, 0):  # the node verdict is advisory: this GPU's own check decides
        t = ctx.submit_jobs(package["multi"], seed=37)
        part, has = ctx.jobs_partial(t)
        assert has and not ctx.final_verify([part])
        got, stats = ctx.wait_jobs_node(t, node_valid)
        check(got, stats, package)


# ---- 5. steady state
def reserve_units(keys):
    """what a set counts toward lsg_reserve's max_pks (include/lodestar_bls.h)"""
    from lodestar_amd._native import PkBits, PkBitsMulti
    if isinstance(keys, PkBitsMulti):
        return 16 + 2 * len(keys.committees) + (len(keys) + 31) // 32
    if isinstance(keys, PkBits):
        return 16 + (len(keys) + 31) // 32
    return len(keys)


def test_steady_state_allocates_nothing(table, package, capfd, monkeypatch):
    from lodestar_amd._native import Context, PkBitsMulti, PreparedJobs
    c = Context(0)
    try:
        table.load(c)
        register_verdict_committees(c)
        only = [([s for s in sets if isinstance(s[0], PkBitsMulti)], f) for sets, f in package["multi"]]
        only = [(sets, f) for sets, f in only if sets]
        for jobs in (package["multi"], only):
            pj = PreparedJobs(jobs)
            n_sets = sum(len(s) for s, _ in jobs)
            c.reserve(n_sets, max_pks=sum(reserve_units(s[0]) for sets, _ in jobs for s in sets), max_msg_bytes=160 * n_sets,
                      n_slots=2)
            want = norm(c.verify_jobs(pj, seed=5)[0])  # warm-up
            monkeypatch.setenv("LSG_TRACE_ALLOC", "1")
            capfd.readouterr()
            before = c.allocation_count()
            assert norm(c.verify_jobs(pj, seed=6)[0]) == want
            trace = [ln for ln in capfd.readouterr().err.splitlines() if "lsg alloc" in ln]
            assert c.allocation_count() == before, trace
            monkeypatch.delenv("LSG_TRACE_ALLOC")
    finally:
        c.close()


# ---- 6. launches
def test_the_new_kernel_runs_only_for_multi_sets(ctx, table, package):
    from lodestar_amd._native import Context, PkBitsMulti
    got_c, stats_c = ctx.verify_jobs(package["index"], seed=41)
    names_c = names(ctx)
    assert names_c and "k_pk_agg_bits_multi" not in names_c
    plain = Context(0)
    try:  # a context that never saw the form or a committee launches the same
        table.load(plain)
        got_p, stats_p = plain.verify_jobs(package["index"], seed=41)
        assert names(plain) == names_c
        assert got_p == got_c and [stats_p[k] for k in COUNTERS] == [stats_c[k] for k in COUNTERS]
    finally:
        plain.close()
    only = [([s for s in sets if isinstance(s[0], PkBitsMulti)], f) for sets, f in package["multi"]]
    only = [(sets, f) for sets, f in only if sets]
    assert sum(len(s) for s, _ in only) == 16
    got, _ = ctx.verify_jobs(only, seed=43)
    assert {g[0] for g in got} == {0, 1}
    got = names(ctx)
    assert "k_pk_agg_bits_multi" in got and "g1_aggregate" not in got and "k_pk_agg_bits" not in got, got


# ---- Node
def test_node_electra_style_package(ctx, table, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: three aggregates spanning
    committees, each as {committees, bits, bitLen}; valid, then with a wrong bit; through
    verifySignatureSets on both verifiers and verifySignatureSetsSameMessage."""
    import json
    import os
    import shutil
    import subprocess
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(os.path.join(here, "..", "lodestar_amd", "napi", "lsg_napi.node")), "N-API addon not built"
    rng = random.Random(21)
    committees = [[rng.randrange(64) for _ in range(n)] for n in (33, 7, 64, 130, 9)]
    lists = [[0, 1, 2], [4, 3], [2, 2, 1, 0, 3]]
    msg = hashlib.sha256(b"lodestar-mi355x" + b"electra-aggregate").digest()
    rows = [[r for k in ks for r in committees[k]] for ks in lists]
    bits = [[1 if rng.random() < 0.95 else 0 for _ in rw] for rw in rows]
    sks = [sum(table.sk[r] for r in bits_of(rw, b)) % R for rw, b in zip(rows, bits)]
    sigs = ctx.sign(sks, [msg] * 3)
    agg = [table.aggregate(bits_of(rw, b))[0] for rw, b in zip(rows, bits)]
    wrong = list(bits[1])
    wrong[wrong.index(1)] = 0
    assert co.verify_each(agg + [table.aggregate(bits_of(rows[1], wrong))[0]], [msg] * 4, sigs + [sigs[1]]) == [1] * 3 + [0]
    cases = {"pks": [k.hex() for k in table.enc[:64]], "first_id": 50, "committees": committees, "msg": msg.hex(),
             "sets": [{"committees": [50 + k for k in lists[i]], "bits": pack(bits[i]).hex(), "bit_len": len(bits[i]),
                       "sig": sigs[i].hex()} for i in range(3)],
             "wrong": {"set": 1, "bits": pack(wrong).hex()}}
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(here, "js", "test_committees_multi_gpu.js"), str(f)], capture_output=True,
                       text=True, timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "committees multi gpu ok" in r.stdout, r.stdout + r.stderr
