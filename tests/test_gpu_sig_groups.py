"""Per-group aggregates of the verified signatures on the GPU (lsg_submit_jobs_grouped /
lsg_wait_jobs_grouped, k_sig_agg_seg).  Every expected aggregate is
Context.aggregate_signatures (lsg_aggregate_signatures, pinned by tests/golden/
aggregate_signatures.json in tests/test_gpu_parity.py) over the signatures of the sets whose job
is LSG_VALID, for a few groups also the oracle's own G2 sum; verdicts, error codes and counters
are compared with the same package through submit_jobs under the same seed.  Every comparison
is exact.  Every test here needs an MI355X.

Keys are the 64 interop keys (and r - sk for a signature's negative); signatures come from
ctx.sign.  The packages hold about 650 sets each: group lengths 0, 1, 2, 31, 32, 33 and 513 --
one more than a chunk of 32 lane pairs x SEG_FOLD = 16 members (lsg_plan.hpp), so the second
pass runs."""
import json
import os
import random
import shutil
import subprocess

import pytest

from oracle.curves import E2, g2_compress, g2_uncompress
from oracle.fields import R
from oracle.interop import interop_secret_key
from tests import blsdata as bd

pytestmark = pytest.mark.gpu
B = 1  # LSG_JOB_BATCHABLE
NO_GROUP = 0xFFFFFFFF
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job")
HERE = os.path.dirname(os.path.abspath(__file__))
TWO_PASS = 32 * 16 + 1
LENGTHS = [0, 1, 2, 31, 32, 33, TWO_PASS]  # groups 0..6
G_TWICE, G_CANCEL, G_CANCEL_BUT_ONE = 7, 8, 9
N_GROUPS = 11  # group 10 stays empty too
INF96 = bytes([0xC0]) + bytes(95)


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def names(c):
    return [k for k, _ in c.last_kernel_times()]


class World:
    """One package of single-set batchable jobs in shuffled order: per set (pk, msg, sig96, sig as
    sent, group).  Every fifth signature is sent in its 192-byte form."""

    def __init__(self, ctx):
        rng = random.Random(77)
        sks = [interop_secret_key(i) for i in range(64)]
        plan = []  # (secret key, message, group)
        i = 0
        for g, ln in enumerate(LENGTHS):
            for _ in range(ln):
                plan.append((sks[i % 64], bd.msg("grp", i), g))
                i += 1
        for _ in range(20):
            plan.append((sks[i % 64], bd.msg("grp", i), NO_GROUP))
            i += 1
        m7, m8, m9, m9b = (bd.msg("grp-special", k) for k in range(4))
        plan += [(sks[3], m7, G_TWICE)] * 2                                   # P + P
        plan += [(sks[5], m8, G_CANCEL), (R - sks[5], m8, G_CANCEL)]          # sigma and -sigma: infinity
        plan += [(sks[6], m9, G_CANCEL_BUT_ONE), (sks[7], m9b, G_CANCEL_BUT_ONE), (R - sks[6], m9, G_CANCEL_BUT_ONE)]
        rng.shuffle(plan)  # interleaved group ids
        self.sk = [p[0] for p in plan]
        self.msg = [p[1] for p in plan]
        self.group = [p[2] for p in plan]
        self.n = len(plan)
        self.pk = ctx.sk_to_pk(self.sk)
        self.sig96 = ctx.sign(self.sk, self.msg)
        wide = ctx.sig_decode(self.sig96)
        assert all(e == 0 for _, e in wide)
        self.sent = [wide[k][0] if k % 5 == 0 else self.sig96[k] for k in range(self.n)]
        self.members = {g: [k for k in range(self.n) if self.group[k] == g] for g in range(N_GROUPS)}
        assert [len(self.members[g]) for g in range(7)] == LENGTHS and self.n < 700
        assert any(len(self.sent[k]) == 192 for k in self.members[2] + self.members[3])

    def sets(self):
        return [([self.pk[k]], self.msg[k], self.sent[k]) for k in range(self.n)]

    def expected(self, ctx, sets, included):
        """[(bytes96, count)] per group over the sets in `included`, from lsg_aggregate_signatures
        over their signatures in compressed form (the same points as the 192-byte forms sent)"""
        mem = [[k for k in self.members[g] if k in included] for g in range(N_GROUPS)]
        ref = ctx.aggregate_signatures([[self.sig96[k] for k in m] for m in mem])
        out = []
        for m, (agg, err) in zip(mem, ref):
            assert err == (0 if m else 101)
            out.append((agg, len(m)) if m else (bytes(96), 0))
        return out


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


def oracle_sum(sigs96):
    acc = None
    for s in sigs96:
        acc = E2.add(acc, g2_uncompress(s))
    return g2_compress(acc)


def test_aggregates_of_a_valid_package(ctx, world):
    w = world
    jobs = [([s], B) for s in w.sets()]
    got, stats, aggs = ctx.verify_jobs_grouped(jobs, w.group, N_GROUPS, seed=11)
    launched = names(ctx)
    assert got == [(1, 0)] * w.n
    assert "k_sig_agg_seg" in launched and "sig_agg_reduce" in launched  # the long group: two passes
    assert launched.count("k_sig_agg_seg") == 1  # every job valid: the sums launched at submit stand
    exp = w.expected(ctx, w.sets(), set(range(w.n)))
    for g in range(N_GROUPS):
        print("group", g, "count", aggs[g][1], "expected", exp[g][1], aggs[g][0][:8].hex(), exp[g][0][:8].hex())
    assert aggs == exp
    assert [n for _, n in aggs] == LENGTHS + [2, 2, 3, 0]
    assert aggs[0] == (bytes(96), 0) and aggs[10] == (bytes(96), 0)
    assert aggs[G_CANCEL] == (INF96, 2)  # a sum at infinity, two signatures summed
    lone = w.members[G_CANCEL_BUT_ONE][[w.msg[k] for k in w.members[G_CANCEL_BUT_ONE]].index(bd.msg("grp-special", 3))]
    assert aggs[G_CANCEL_BUT_ONE] == (w.sig96[lone], 3)
    # the oracle's own G2 arithmetic for the short groups, the doubling and the cancellation
    for g in (1, 2, G_TWICE, G_CANCEL):
        assert aggs[g][0] == oracle_sum([w.sig96[k] for k in w.members[g]]), g
    # nothing else changes: the same package through submit_jobs under the same seed
    plain, pstats = ctx.verify_jobs(jobs, seed=11)
    assert plain == got and [stats[k] for k in COUNTERS] == [pstats[k] for k in COUNTERS]
    assert stats["n_final_exps"] == pstats["n_final_exps"]


def spoiled(ctx, w):
    """The package with sets that do not verify: (jobs, groups, per-job expectation: True when
    every set of the job is good).  Bad sets: a forged one (wrong message), an undecodable
    signature, the off-curve point of tests/golden/mainnet_g2_points_bad.json, a point on the
    curve but outside the subgroup, a three-set job with one forged set, and non-batchable jobs
    (one good, one forged)."""
    sets = w.sets()
    bad = set()

    def spoil(g, at, how):
        k = w.members[g][at]
        sets[k] = how(sets[k])
        bad.add(k)
        return k

    spoil(3, 4, bd.corrupt_wrong_message)
    spoil(4, 9, bd.corrupt_flip_x_bit)
    off_curve = bytes.fromhex(json.load(open(os.path.join(HERE, "golden", "mainnet_g2_points_bad.json")))[0]["sig"])
    spoil(5, 1, lambda s: (s[0], s[1], off_curve))
    spoil(5, 20, bd.corrupt_not_in_group)
    spoil(6, 300, bd.corrupt_wrong_message)
    # jobs: a three-set job (members of groups 6, 2 and 6; the last one forged), a good and a
    # forged two-set non-batchable job over members of group 6, the rest single-set batchable
    trio = [w.members[6][10], w.members[2][0], w.members[6][11]]
    sets[trio[2]] = bd.corrupt_wrong_message(sets[trio[2]])
    bad.add(trio[2])
    nb_good = [w.members[6][20], w.members[6][21]]
    nb_bad = [w.members[6][30], w.members[6][31]]
    sets[nb_bad[0]] = bd.corrupt_wrong_message(sets[nb_bad[0]])
    bad.add(nb_bad[0])
    multi = {k for job in (trio, nb_good, nb_bad) for k in job}
    job_sets = [[k] for k in range(w.n) if k not in multi]
    flags = [B] * len(job_sets)
    job_sets[100:100] = [trio]
    flags[100:100] = [B]
    job_sets[200:200] = [nb_good]
    flags[200:200] = [0]
    job_sets += [nb_bad]
    flags += [0]
    jobs = [([sets[k] for k in js], f) for js, f in zip(job_sets, flags)]
    groups = [w.group[k] for js in job_sets for k in js]
    good_job = [all(k not in bad for k in js) for js in job_sets]
    return sets, jobs, groups, job_sets, good_job


def test_sets_that_did_not_verify_are_left_out(ctx, world):
    w = world
    sets, jobs, groups, job_sets, good_job = spoiled(ctx, w)
    got, stats, aggs = ctx.verify_jobs_grouped(jobs, groups, N_GROUPS, seed=13)
    launched = names(ctx)
    assert [g[0] == 1 for g in got] == good_job
    assert sum(1 for g in got if g[0] == 2) == 3  # undecodable, off the curve, outside the subgroup
    assert launched.count("k_sig_agg_seg") == 2  # planned again over the included sets
    included = {k for js, ok in zip(job_sets, good_job) if ok for k in js}
    assert len(included) == w.n - 10  # seven bad sets, and the three good sets of the two failed multi-set jobs
    exp = w.expected(ctx, sets, included)
    for g in range(N_GROUPS):
        print("group", g, "count", aggs[g][1], "expected", exp[g][1], aggs[g][0][:8].hex(), exp[g][0][:8].hex())
    assert aggs == exp
    assert [n for _, n in aggs] == [0, 1, 1, 30, 31, 31, TWO_PASS - 5, 2, 2, 3, 0]
    plain, pstats = ctx.verify_jobs(jobs, seed=13)
    assert plain == got and [stats[k] for k in COUNTERS] == [pstats[k] for k in COUNTERS]
    assert stats["n_final_exps"] == pstats["n_final_exps"]


def test_a_package_rejected_by_a_key_error_includes_nothing(ctx, world):
    w = world
    sets = w.sets()[:80]
    sets[17] = ([bytes([0xFF] * 96)], sets[17][1], sets[17][2])  # a key that does not deserialize
    jobs = [([s], B) for s in sets]
    groups = [k % 4 for k in range(80)]
    got, stats, aggs = ctx.verify_jobs_grouped(jobs, groups, 4, seed=17)
    assert all(g[0] == 2 for g in got) and stats["key_error"] != 0 and stats["key_error_job"] == 17
    assert aggs == [(bytes(96), 0)] * 4
    plain, pstats = ctx.verify_jobs(jobs, seed=17)
    assert plain == got and [stats[k] for k in COUNTERS] == [pstats[k] for k in COUNTERS]


def test_plain_forms(ctx, world):
    import ctypes
    from lodestar_amd._native import PreparedJobs
    w = world
    jobs = [([s], B) for s in w.sets()[:90]]
    groups = [k % 3 for k in range(90)]
    ref, rstats = ctx.verify_jobs(jobs, seed=19)
    plain_names = names(ctx)
    assert "k_sig_agg_seg" not in plain_names
    # set_group == NULL and n_groups == 0 are lsg_submit_jobs
    p = PreparedJobs(jobs)
    ids = (ctypes.c_uint32 * 90)(*groups)
    for set_group, n_groups in ((None, 3), (ids, 0)):
        raw = ctypes.c_uint64()
        ctx._check(ctx.lib.lsg_submit_jobs_grouped(ctx.h, p.jobs, p.n_jobs, 19, set_group, n_groups, ctypes.byref(raw)),
                   "lsg_submit_jobs_grouped")
        got, stats, aggs = ctx.wait_jobs_grouped((raw.value, p.n_jobs))  # on a plain ticket: no aggregate
        assert (got, aggs) == (ref, []) and [stats[k] for k in COUNTERS] == [rstats[k] for k in COUNTERS]
        assert names(ctx) == plain_names
    # a grouped ticket: poll works, and wait_jobs resolves it (the aggregates are dropped)
    t = ctx.submit_jobs(jobs, seed=19, groups=groups, n_groups=3)
    assert t.n_groups == 3 and (t[0] >> 8) & 255 == 1
    while not ctx.poll(t):
        pass
    got, stats = ctx.wait_jobs(t)
    assert got == ref and [stats[k] for k in COUNTERS] == [rstats[k] for k in COUNTERS]
    assert "k_sig_agg_seg" in names(ctx)
    # and the grouped pair gives the same verdicts plus the aggregates
    got, stats, aggs = ctx.verify_jobs_grouped(jobs, groups, 3, seed=19)
    assert got == ref and [n for _, n in aggs] == [30, 30, 30]
    assert aggs == [(a, 30) for a, _ in ctx.aggregate_signatures([[w.sig96[k] for k in range(g, 90, 3)] for g in range(3)])]


def test_argument_and_context_errors(ctx, world):
    from lodestar_amd._native import Context
    w = world
    jobs = [([s], B) for s in w.sets()[:40]]
    for bad in (2, 3, NO_GROUP - 1):
        groups = [k % 2 for k in range(40)]
        groups[33] = bad
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            ctx.submit_jobs(jobs, seed=23, groups=groups, n_groups=2)
        got, _, aggs = ctx.verify_jobs_grouped(jobs, [k % 2 for k in range(40)], 2, seed=23)  # the context stays usable
        assert got == [(1, 0)] * 40 and [n for _, n in aggs] == [20, 20]
    with pytest.raises(ValueError):
        ctx.submit_jobs(jobs, seed=23, groups=[0] * 39, n_groups=2)
    c2 = Context(devices=[0, 0])
    try:
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            c2.submit_jobs(jobs, seed=23, groups=[0] * 40, n_groups=1)
        assert c2.verify_jobs(jobs, seed=23)[0] == [(1, 0)] * 40
        assert c2.verify_jobs_grouped(jobs, None, 0, seed=23)[0] == [(1, 0)] * 40
    finally:
        c2.close()


def test_a_grouped_package_is_never_coalesced(world):
    from lodestar_amd._native import Context
    w = world
    sets = w.sets()
    c = Context(0)
    try:
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        held_jobs = [[([sets[k]], B) for k in range(a, a + 8)] for a in (0, 8, 16)]
        held_jobs[1][3] = ([bd.corrupt_wrong_message(sets[11])], B)
        held = [c.submit_jobs(j, seed=29) for j in held_jobs]
        assert all(t is not None and (t[0] >> 8) & 255 == 4 for t in held)  # coalesced tickets
        jobs = [([sets[k]], B) for k in range(100, 160)]
        t = c.submit_jobs(jobs, seed=29, groups=[k % 5 for k in range(60)], n_groups=5)
        assert (t[0] >> 8) & 255 == 1  # a package ticket of its own
        got, _, aggs = c.wait_jobs_grouped(t)
        assert got == [(1, 0)] * 60
        assert aggs == [(a, 12) for a, _ in c.aggregate_signatures([[w.sig96[100 + k] for k in range(g, 60, 5)] for g in range(5)])]
        res = [c.wait_jobs(t)[0] for t in held]
        assert res[0] == [(1, 0)] * 8 and res[2] == [(1, 0)] * 8
        assert res[1] == [(1, 0)] * 3 + [(0, 0)] + [(1, 0)] * 4
    finally:
        c.close()


def test_reserved_context_allocates_nothing(world):
    from lodestar_amd._native import Context, PreparedJobs
    w = world
    sets = w.sets()[:300]
    c = Context(0)
    try:
        c.reserve(300, max_pks=300, max_msg_bytes=32 * 300, n_slots=2)
        good = PreparedJobs([([s], B) for s in sets])
        forged = list(sets)
        forged[123] = bd.corrupt_wrong_message(forged[123])
        forged = PreparedJobs([([s], B) for s in forged])
        groups = [k % 7 if k % 11 else NO_GROUP for k in range(300)]
        first = c.verify_jobs_grouped(good, groups, 7, seed=31)  # the first grouped package allocates
        c.reserve(300, max_pks=300, max_msg_bytes=32 * 300, n_slots=2)  # ... and the caller reserves again
        c.verify_jobs_grouped(forged, groups, 7, seed=31)  # warm-up of the fallback phases
        before = c.allocation_count()
        for k in range(10):
            pkg = forged if k % 2 else good
            got, _, aggs = c.verify_jobs_grouped(pkg, groups, 7, seed=32 + k)
            assert [g[0] for g in got].count(1) == (299 if k % 2 else 300)
            if not k % 2:
                assert aggs == first[2]
        assert c.allocation_count() == before
    finally:
        c.close()


def test_node_handler_gets_the_aggregates(ctx, world, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: the onAggregates entries equal
    aggregateSignatures over the sets that resolved true (tests/js/test_aggregate_gpu.js)."""
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    assert os.path.exists(os.path.join(HERE, "..", "lodestar_amd", "napi", "lsg_napi.node")), "N-API addon not built"
    w = world
    ks = w.members[3] + w.members[4] + w.members[1] + w.members[G_CANCEL] + w.members[5][:5]  # (group 5: sent without a key)
    sets = w.sets()
    forged = {ks[2], ks[40]}
    cases = {"sets": [{"pk": sets[k][0][0].hex(), "msg": (bd.corrupt_wrong_message(sets[k]) if k in forged else sets[k])[1].hex(),
                       "sig": sets[k][2].hex(), "sig96": w.sig96[k].hex(), "key": "group-%d" % w.group[k] if w.group[k] != 5 else None,
                       "tag": k} for k in ks],
             "forged": sorted(ks.index(k) for k in forged), "cancel_key": "group-%d" % G_CANCEL}
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_aggregate_gpu.js"), str(f)], capture_output=True, text=True,
                       timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "aggregate gpu ok" in r.stdout, r.stdout + r.stderr
