"""Committee-resident keys on the GPU: lsg_committees_set and sets given as
committee id + participation bits (LSG_PK_BITS, k_pk_agg_bits), against the same sets given
by table index, the Python oracle's PublicKey.aggregate and tests/cpu_oracle.py's worker.ts
rules.  Every comparison is exact (bytes and integers).  Every test here needs an MI355X.

The table has 600 rows: the keys of secret keys 1..64 repeated, the infinity key at row 100,
row 200 left unset, and P / -P (secret key 8; -P is P's compressed encoding with the sign bit
flipped) at rows 300 / 301.
"""
import hashlib
import random

import pytest

from oracle import verifier as ov
from oracle.curves import g1_compress, g1_deserialize, g1_serialize
from oracle.fields import R
from tests import cpu_oracle as co

pytestmark = pytest.mark.gpu
B, V = 1, 4  # LSG_JOB_BATCHABLE, LSG_JOB_VALIDATE_KEYS
ROWS, ROW_INF, ROW_UNSET, ROW_P, ROW_NEG_P = 600, 100, 200, 300, 301
INF96 = bytes([0x40]) + bytes(95)
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 450, 512, 513, 2048, 2049]
ERR_EMPTY_AGGREGATE, ERR_BAD_INDEX, ERR_BAD_COMMITTEE = 101, 102, 103
# special committees (ids 900..): members are table rows
DUP = [5, 5, 5, 9, 9, ROW_P, 5]
WITH_INF = [ROW_INF, 1, 2, ROW_INF, 3]
P_NEG_P = [ROW_P, ROW_NEG_P]
MIXED_SIGNS = [1, ROW_P, 2, ROW_NEG_P, 3]
CANCEL_BUT_ONE = [ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, 7]
NEG_SUM = [ROW_P, ROW_NEG_P, ROW_NEG_P, ROW_P, ROW_NEG_P]
SUM_INF = [ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P, ROW_P, ROW_NEG_P]
SPECIAL = [DUP, WITH_INF, P_NEG_P, MIXED_SIGNS, CANCEL_BUT_ONE, NEG_SUM, SUM_INF]
FIRST_LEN_ID, FIRST_SPECIAL_ID, FIRST_VERDICT_ID = 10, 900, 2000


class Table:
    """the fixture table, host side: per row its encoded key, oracle point and secret key"""

    def __init__(self, ctx):
        pks = ctx.sk_to_pk(list(range(1, 65)))
        self.enc = [pks[r % 64] for r in range(ROWS)]
        self.sk = [r % 64 + 1 for r in range(ROWS)]
        self.enc[ROW_INF], self.sk[ROW_INF] = INF96, 0
        p48 = g1_compress(g1_deserialize(pks[7]))
        self.p48 = [p48, bytes([p48[0] ^ 0x20]) + p48[1:]]
        self.sk[ROW_P], self.sk[ROW_NEG_P] = 8, R - 8
        self.enc[ROW_P], self.enc[ROW_NEG_P] = (g1_serialize(g1_deserialize(b)) for b in self.p48)
        self.pt = [g1_deserialize(b) for b in self.enc]
        self.enc[ROW_UNSET] = self.pt[ROW_UNSET] = self.sk[ROW_UNSET] = None

    def load(self, ctx):
        assert ctx.pubkey_table_set(0, self.enc[:ROW_UNSET]) == [0] * ROW_UNSET
        assert ctx.pubkey_table_set(ROW_UNSET + 1, self.enc[ROW_UNSET + 1:ROW_P]) == [0] * (ROW_P - ROW_UNSET - 1)
        assert ctx.pubkey_table_set(ROW_P, self.p48) == [0, 0]
        assert ctx.pubkey_table_set(ROW_NEG_P + 1, self.enc[ROW_NEG_P + 1:]) == [0] * (ROWS - ROW_NEG_P - 1)
        assert ctx.pubkey_table_size() == ROWS

    def aggregate(self, rows):
        """the oracle's PublicKey.aggregate of the rows' keys: (96 bytes, code)"""
        if not rows:
            return INF96, ERR_EMPTY_AGGREGATE
        return g1_serialize(ov.aggregate_pubkeys([self.pt[r] for r in rows])), 0


def pack(bits, garbage=None):
    raw = bytearray((len(bits) + 7) // 8)
    for k, b in enumerate(bits):
        if b:
            raw[k >> 3] |= 1 << (k & 7)
    if garbage is not None:  # noise in the padding bits
        for k in range(len(bits), 8 * len(raw)):
            if garbage.random() < 0.7:
                raw[k >> 3] |= 1 << (k & 7)
    return bytes(raw)


def patterns(n, rng):
    out = [[0] * n, [1] + [0] * (n - 1), [0] * (n - 1) + [1], [1] * n, [1] * n,
           [1 if k < n // 2 else 0 for k in range(n)], [k & 1 for k in range(n)]]
    out[4][rng.randrange(n)] = 0
    rng.shuffle(out[5])
    out += [[1 if rng.random() < q else 0 for _ in range(n)] for q in (0.01, 0.5, 0.99)]
    return out


def usable_rows(rng, n):
    """n members drawn from the rows that hold a key (the infinity key and P / -P included)"""
    rows = [r for r in range(ROWS) if r != ROW_UNSET]
    return [rng.choice(rows) for _ in range(n)]


def length_committees():
    rng = random.Random(811)
    return [usable_rows(rng, n) for n in LENGTHS]


def register(ctx):
    """the committees every test uses: one per length (ids 10..), the special ones (900..)"""
    lens = length_committees()
    assert ctx.committees_set(FIRST_LEN_ID, lens) == [0] * len(lens)
    assert ctx.committees_set(FIRST_SPECIAL_ID, SPECIAL) == [0] * len(SPECIAL)
    assert ctx.committee_count() == FIRST_SPECIAL_ID + len(SPECIAL)
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


def bits_of(rows, bits):
    return [r for r, b in zip(rows, bits) if b]


# ---- 1. aggregates
def test_aggregates_match_index_sets_and_oracle(ctx, table):
    from lodestar_amd._native import PkBits, PkIndices
    rng = random.Random(5)
    cases = []  # (committee id, rows, bits)
    for k, rows in enumerate(length_committees()):
        cases += [(FIRST_LEN_ID + k, rows, bits) for bits in patterns(len(rows), rng)]
    for k, rows in enumerate(SPECIAL):
        cases += [(FIRST_SPECIAL_ID + k, rows, bits) for bits in ([1] * len(rows), [0] + [1] * (len(rows) - 1))]
    sid = {name: FIRST_SPECIAL_ID + k for k, name in enumerate(
        ["dup", "with_inf", "p_neg_p", "mixed_signs", "cancel_but_one", "neg_sum", "sum_inf"])}
    cases += [
        (sid["mixed_signs"], MIXED_SIGNS, [0, 1, 0, 1, 0]),            # participants P, -P: the identity (direct)
        (sid["cancel_but_one"], CANCEL_BUT_ONE, [1, 1, 1, 1, 1, 1, 0]),  # complement: absentees == sum
        (sid["neg_sum"], NEG_SUM, [0, 1, 1, 1, 1]),                    # complement: absentees == -sum
        (sid["sum_inf"], SUM_INF, [0, 1, 1, 1, 1, 1]),                 # complement: the sum is the identity
        (sid["with_inf"], WITH_INF, [1, 0, 0, 1, 0]),                  # only infinity keys take part
        (sid["dup"], DUP, [1, 1, 0, 1, 0, 0, 1]),
    ]
    want = [table.aggregate(bits_of(rows, bits)) for _, rows, bits in cases]
    by_bits = ctx.aggregate_pubkeys_multi([PkBits(cid, pack(bits, rng), len(bits)) for cid, _, bits in cases])
    names = [k for k, _ in ctx.last_kernel_times()]
    assert "k_pk_agg_bits" in names and "g1_aggregate" not in names, names  # no k_pk_agg_seg pass
    by_index = ctx.aggregate_pubkeys_multi([PkIndices(bits_of(rows, bits)) for _, rows, bits in cases])
    names = [k for k, _ in ctx.last_kernel_times()]
    assert "g1_aggregate" in names and "k_pk_agg_bits" not in names, names
    bad = [(i, cases[i][0], len(cases[i][1]), sum(cases[i][2])) for i in range(len(cases))
           if not (by_bits[i] == by_index[i] == want[i])]
    assert not bad, bad[:10]
    # the named special results, whatever the three agree on
    neg2p = g1_serialize(ov.sk_to_pk(R - 16))
    assert [w[0] for w in want[-6:-2]] == [INF96, INF96, neg2p, table.enc[ROW_NEG_P]]
    assert table.aggregate(P_NEG_P)[0] == INF96
    # a call mixing the three forms: each set takes its own path
    mixed = ctx.aggregate_pubkeys_multi([PkBits(sid["dup"], pack([1] * 7), 7), PkIndices(DUP), [table.enc[r] for r in DUP]])
    assert mixed == [table.aggregate(DUP)] * 3
    names = [k for k, _ in ctx.last_kernel_times()]
    assert "k_pk_agg_bits" in names and "g1_aggregate" in names, names
    # the single-list call does not know the form
    out, err = ctx.aggregate_pubkeys([bytes(8)] * 2)
    assert err == 10  # BLST_INVALID_SIZE, as for any unknown key length


# ---- 2. verdicts
def verdict_package(ctx, table):
    """Jobs of 1-3 sets mixing byte, index and bits sets, batchable and not; some forged.
    Returns (jobs with bits sets, the same with index sets, per-set oracle outcomes)."""
    from lodestar_amd._native import PkBits, PkIndices
    rng = random.Random(99)
    committees = [usable_rows(rng, n) for n in (3, 17, 64, 130, 450)]
    assert ctx.committees_set(FIRST_VERDICT_ID, committees) == [0] * len(committees)
    sets = []  # (form, committee k, claimed bits, msg, sig)
    n_sets = 44
    for i in range(n_sets):
        k = i % len(committees)
        n = len(committees[k])
        q = [0.99, 0.9, 0.5][i % 3]
        bits = [1 if rng.random() < q else 0 for _ in range(n)]
        bits[rng.randrange(n)] = 1
        msg = hashlib.sha256(b"lodestar-mi355x" + b"committee" + i.to_bytes(8, "little")).digest()
        sets.append([("bits", "index", "bytes", "bits")[i % 4], k, bits, msg, None])
    sks = [sum(table.sk[r] for r in bits_of(committees[k], bits)) % R for _, k, bits, _, _ in sets]
    for st, sig in zip(sets, ctx.sign(sks, [st[3] for st in sets])):
        st[4] = sig
    forged = {}
    for i, kind in ((4, "wrong_bit"), (12, "absentee"), (19, "signature"), (28, "wrong_bit"), (41, "absentee")):
        _, k, bits, _, _ = sets[i]
        if kind == "signature":
            sets[i][4] = sets[i + 1][4]  # decodes, does not verify
        else:
            flip = [j for j, b in enumerate(bits) if b == (1 if kind == "wrong_bit" else 0)
                    and table.sk[committees[k][j]] != 0]
            if not flip:  # (nothing absent: clear a bit instead)
                flip = [j for j, b in enumerate(bits) if b and table.sk[committees[k][j]] != 0]
            bits[flip[0]] ^= 1
        forged[i] = kind
    as_bits, as_index, agg = [], [], []
    for form, k, bits, msg, sig in sets:
        rows = bits_of(committees[k], bits)
        agg.append(table.aggregate(rows)[0])
        alt = {"bits": PkBits(FIRST_VERDICT_ID + k, pack(bits), len(bits)), "index": PkIndices(rows),
               "bytes": [table.enc[r] for r in rows]}
        as_bits.append((alt[form], msg, sig))
        as_index.append((alt["index" if form == "bits" else form], msg, sig))
    per_set = co.verify_each(agg, [s[3] for s in sets], [s[4] for s in sets])
    assert [i for i, v in enumerate(per_set) if v != 1] == sorted(forged), (per_set, forged)
    shape, pos = [], 0
    while pos < n_sets:
        cnt = min(1 + len(shape) % 3, n_sets - pos)
        shape.append((pos, cnt, B if len(shape) % 5 != 3 else 0))
        pos += cnt

    def jobs(flat):
        return [(flat[p:p + c], f) for p, c, f in shape]
    return jobs(as_bits), jobs(as_index), per_set


def expected(jobs, per_set):
    jsets, pos = [], 0
    for sets, _ in jobs:
        jsets.append(list(range(pos, pos + len(sets))))
        pos += len(sets)
    return co.expected_jobs(jsets, [bool(f & B) for _, f in jobs], per_set)


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job")


@pytest.fixture(scope="module")
def package(ctx, table):
    jb, ji, per_set = verdict_package(ctx, table)
    exp, retries, success = expected(jb, per_set)
    assert {e[0] for e in exp} == {0, 1}
    return {"bits": jb, "index": ji, "exp": exp, "retries": retries, "success": success}


def check(got, stats, package, counters=True):
    assert norm(got) == package["exp"]
    assert stats["key_error"] == 0
    if counters:
        assert (stats["batch_retries"], stats["batch_sigs_success"]) == (package["retries"], package["success"]), stats


def test_verdicts_of_a_mixed_package(ctx, package):
    got_b, stats_b = ctx.verify_jobs(package["bits"], seed=3)
    names = [k for k, _ in ctx.last_kernel_times()]
    assert "k_pk_agg_bits" in names and "g1_aggregate" in names, names  # bits and ordinary sets, each its own way
    check(got_b, stats_b, package)
    got_i, stats_i = ctx.verify_jobs(package["index"], seed=3)
    assert "k_pk_agg_bits" not in [k for k, _ in ctx.last_kernel_times()]
    assert got_b == got_i
    assert [stats_b[k] for k in COUNTERS] == [stats_i[k] for k in COUNTERS]
    # one job of bits sets through maybeBatch (lsg_verify_sets), valid and forged
    flat = [s for sets, _ in package["bits"] for s in sets]
    assert ctx.verify_sets([flat[0], flat[3], flat[7]]) == (1, 0)
    assert ctx.verify_sets([flat[0], flat[4], flat[7]]) == (0, 0)
    # lsg_batch_partial: the shard of bits sets alone
    from lodestar_amd._native import PkBits
    only = [s for s in flat if isinstance(s[0], PkBits)]
    good = [s for s in only if s not in (flat[4], flat[12], flat[19], flat[28])]
    part, errs, anyerr = ctx.batch_partial(good, seed=8)
    assert not anyerr and errs == [0] * len(good) and ctx.final_verify([part])
    part, errs, anyerr = ctx.batch_partial(only, seed=8)
    assert not anyerr and not ctx.final_verify([part])


# ---- 3. errors
def test_errors_and_stale_committees(table):
    from lodestar_amd._native import Context, PkBits
    c = Context(0)
    try:
        table.load(c)
        good_rows, stale_rows = [1, 2, 3, 4, 5, 6, 7, 8, 9], [20, 21, 22, 23]
        errs = c.committees_set(0, [good_rows, [1, ROW_UNSET, 2], [], stale_rows])
        assert errs == [0, ERR_BAD_INDEX, ERR_EMPTY_AGGREGATE, 0]
        assert c.committee_count() == 4
        msgs = [hashlib.sha256(b"lodestar-mi355x" + b"cm-errors" + bytes([i])).digest() for i in range(4)]

        def signed(cid, rows, bits, msg, n_bits=None):
            sk = sum(table.sk[r] for r in bits_of(rows, bits)) % R
            return (PkBits(cid, pack(bits), len(bits) if n_bits is None else n_bits), msg, c.sign([sk or 1], [msg])[0])
        full9, full4 = [1] * 9, [1] * 4
        ok = [signed(0, good_rows, full9, msgs[0]), signed(0, good_rows, [1, 0, 1, 1, 1, 1, 1, 1, 1], msgs[1]),
              signed(3, stale_rows, full4, msgs[2])]

        def run(third, flags=B):
            return c.verify_jobs([([ok[0]], B), ([ok[1]], flags), ([third], B), ([ok[2]], 0)], seed=17)
        got, stats = run(ok[0])
        assert norm(got) == [(1, 0)] * 4 and stats["key_error"] == 0
        for bad in (signed(77, good_rows, full9, msgs[3]),             # unknown id
                    signed(0, good_rows, full9, msgs[3], n_bits=10),   # length mismatch
                    signed(0, good_rows, full9[:8], msgs[3]),
                    signed(1, [1, 2, 3], [1, 1, 1], msgs[3]),          # left unset: names the unset row
                    signed(2, [], [], msgs[3])):                       # left unset: empty
            got, stats = run(bad)
            assert (stats["key_error"], stats["key_error_job"]) == (ERR_BAD_COMMITTEE, 2), stats
            assert norm(got) == [(2, ERR_BAD_COMMITTEE)] * 4
            assert c.aggregate_pubkeys_multi([bad[0], ok[0][0]])[0][1] == ERR_BAD_COMMITTEE
            part, errs, anyerr = c.batch_partial([ok[0], bad], seed=2)
            assert anyerr and errs == [0, ERR_BAD_COMMITTEE]
        # no participant: EMPTY_AGGREGATE_ARRAY for its job only
        empty = (PkBits(0, bytes(2), 9), msgs[3], ok[0][2])
        got, stats = run(empty)
        assert norm(got) == [(1, 0), (1, 0), (2, ERR_EMPTY_AGGREGATE), (1, 0)] and stats["key_error"] == 0
        assert c.aggregate_pubkeys_multi([empty[0]]) == [(INF96, ERR_EMPTY_AGGREGATE)]
        # LSG_JOB_VALIDATE_KEYS leaves bits sets alone
        plain = run(ok[0])
        flagged = run(ok[0], flags=B | V)
        assert flagged[0] == plain[0] and [flagged[1][k] for k in COUNTERS] == [plain[1][k] for k in COUNTERS]
        assert not [k for k, _ in c.last_kernel_times() if "keyvalidate" in k]
        # an append leaves committees set; a rewrite of any row unsets every one of them
        assert c.pubkey_table_set(ROWS, [table.enc[3]]) == [0]
        assert c.committee_count() == 4 and norm(run(ok[0])[0]) == [(1, 0)] * 4
        assert c.pubkey_table_set(21, [table.enc[21]]) == [0]
        assert c.committee_count() == 0
        got, stats = run(ok[0])
        assert (stats["key_error"], stats["key_error_job"]) == (ERR_BAD_COMMITTEE, 0)
        assert c.committees_set(0, [good_rows]) == [0] and c.committees_set(3, [stale_rows]) == [0]
        assert norm(run(ok[0])[0]) == [(1, 0)] * 4
        # a replaced committee answers with its new members; a cleared one is unknown
        assert c.committees_set(3, [good_rows]) == [0]
        assert c.aggregate_pubkeys_multi([PkBits(3, pack(full9), 9)]) == [table.aggregate(good_rows)]
        c.committees_clear(3, 1)
        assert c.committee_count() == 1
        assert c.aggregate_pubkeys_multi([PkBits(3, pack(full9), 9)])[0][1] == ERR_BAD_COMMITTEE
        # the limits
        for first, lists in ((1 << 20, [[1]]), ((1 << 20) - 1, [[1], [2]])):
            with pytest.raises(RuntimeError):
                c.committees_set(first, lists)
        with pytest.raises(RuntimeError):
            c.committees_set(5, [[1] * 131073])
        assert c.committees_set((1 << 20) - 1, [[1, 2]]) == [0] and c.committee_count() == 1 << 20
    finally:
        c.close()


# ---- 4. everywhere jobs go
def test_coalesced_packages(table, package):
    from lodestar_amd._native import Context
    c = Context(0)
    try:
        table.load(c)
        register(c)
        verdict_package(c, table)  # (registers the package's committees on this context)
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        tickets = [c.submit_jobs(p, seed=29) for p in (package["bits"], package["index"], package["bits"])]
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
        register(c)
        verdict_package(c, table)
        got, stats = c.verify_jobs(package["bits"], seed=31)
        check(got, stats, package, counters=False)  # (chunks are formed per device)
        got_i, _ = c.verify_jobs(package["index"], seed=31)
        assert got == got_i
    finally:
        c.close()


def test_node_protocol(ctx, package):
    good = [(sets, f) for (sets, f), e in zip(package["bits"], package["exp"]) if e == (1, 0)]
    t = ctx.submit_jobs(good, seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and ctx.final_verify([part])
    got, _ = ctx.wait_jobs_node(t, 1)
    assert norm(got) == [(1, 0)] * len(good)
    for node_valid in (1, 0):  # the node verdict is advisory: this GPU's own check decides
        t = ctx.submit_jobs(package["bits"], seed=37)
        part, has = ctx.jobs_partial(t)
        assert has and not ctx.final_verify([part])
        got, stats = ctx.wait_jobs_node(t, node_valid)
        check(got, stats, package)


# ---- 5. steady state
def test_steady_state_allocates_nothing(table, package, capfd, monkeypatch):
    from lodestar_amd._native import Context, PkBits, PreparedJobs
    c = Context(0)
    try:
        table.load(c)
        register(c)
        verdict_package(c, table)
        pj = PreparedJobs(package["bits"])
        n_sets = sum(len(s) for s, _ in package["bits"])
        keys = sum(16 + (len(s[0]) + 31) // 32 if isinstance(s[0], PkBits) else len(s[0])
                   for sets, _ in package["bits"] for s in sets)
        c.reserve(n_sets, max_pks=keys, n_slots=2)
        assert norm(c.verify_jobs(pj, seed=5)[0]) == package["exp"]  # warm-up
        monkeypatch.setenv("LSG_TRACE_ALLOC", "1")
        capfd.readouterr()
        before = c.allocation_count()
        assert norm(c.verify_jobs(pj, seed=6)[0]) == package["exp"]
        trace = [ln for ln in capfd.readouterr().err.splitlines() if "lsg alloc" in ln]
        assert c.allocation_count() == before, trace
    finally:
        c.close()


# ---- 6. existing paths untouched
def test_packages_without_bits_sets_launch_what_they_did(ctx, table, package):
    from lodestar_amd._native import Context
    plain = Context(0)
    try:
        table.load(plain)
        assert plain.committee_count() == 0
        got_p, stats_p = plain.verify_jobs(package["index"], seed=41)
        names_p = [k for k, _ in plain.last_kernel_times()]
        got_c, stats_c = ctx.verify_jobs(package["index"], seed=41)
        names_c = [k for k, _ in ctx.last_kernel_times()]
        assert names_p and names_p == names_c and "k_pk_agg_bits" not in names_p
        assert got_p == got_c and [stats_p[k] for k in COUNTERS] == [stats_c[k] for k in COUNTERS]
    finally:
        plain.close()


# ---- Node
def test_node_sync_style_package_by_bits(ctx, table, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: four subcommittee sets over one
    message, each as {committee, bits, bitLen}; valid, then with a wrong bit."""
    import json
    import os
    import shutil
    import subprocess
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(os.path.join(here, "..", "lodestar_amd", "napi", "lsg_napi.node")), "N-API addon not built"
    rng = random.Random(12)
    committees = [[rng.randrange(64) for _ in range(128)] for _ in range(4)]  # (duplicates, as a sync committee has)
    msg = hashlib.sha256(b"lodestar-mi355x" + b"sync-aggregate").digest()
    bits = [[1 if rng.random() < 0.95 else 0 for _ in range(128)] for _ in range(4)]
    sks = [sum(table.sk[r] for r in bits_of(c, b)) % R for c, b in zip(committees, bits)]
    sigs = ctx.sign(sks, [msg] * 4)
    agg = [table.aggregate(bits_of(c, b))[0] for c, b in zip(committees, bits)]
    wrong = list(bits[2])
    wrong[wrong.index(1)] = 0
    assert co.verify_each(agg + [table.aggregate(bits_of(committees[2], wrong))[0]], [msg] * 5, sigs + [sigs[2]]) == [1] * 4 + [0]
    cases = {"pks": [k.hex() for k in table.enc[:64]], "first_id": 50, "committees": committees, "msg": msg.hex(),
             "sets": [{"committee": 50 + k, "bits": pack(bits[k]).hex(), "bit_len": 128, "sig": sigs[k].hex()} for k in range(4)],
             "wrong": {"set": 2, "bits": pack(wrong).hex()}}
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(here, "js", "test_committees_gpu.js"), str(f)], capture_output=True,
                       text=True, timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "committees gpu ok" in r.stdout, r.stdout + r.stderr
