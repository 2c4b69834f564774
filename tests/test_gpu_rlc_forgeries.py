"""Cancelling forgeries in every group structure of a package.  Every corruption of
tests/blsdata.py makes one set invalid on its own; the two kinds here are pairs of sets that an
UNRANDOMISED product check accepts (tests/test_gpu_rlc_edges.py shows that on the device: equal
randomizers pass them, distinct ones do not), so only the random linear combination, and the
rule that an unscaled set (r_i = 0) never shares a check, rejects them:

    offset pair        (pk_a, m_a, sig_a + D) and (pk_b, m_b, sig_b - D), D in G2
    same-message swap  (pk_a, m, sig_b) and (pk_b, m, sig_a)

Expected verdicts and both batch counters come from tests/cpu_oracle.py expected_jobs
(worker.ts:30-106) with the forged sets' outcomes from the C oracle (each is invalid) and the
untouched device-signed sets valid by construction: every job holding a forged set is
LSG_INVALID, every other job LSG_VALID.  Each case runs under two nonzero seeds and under
seed 0 (randomizers from the OS).  Every test here needs an MI355X.
"""
import pytest

from oracle.curves import E2, g2_compress, g2_uncompress
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests.test_gpu_rlc_edges import N_KEYS, offset_pair, single_sets, swapped_pair

pytestmark = pytest.mark.gpu
B = 1  # LSG_JOB_BATCHABLE
SEEDS = (0x5EED01, 0x5EED02, 0)
KINDS = ("offset", "swap")


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


@pytest.fixture(scope="module")
def valid(ctx, keys):
    """device-signed valid sets on distinct messages, shared by the cases (never changed)"""
    return tuple(single_sets(ctx, keys, "rlc-forge", 300))


@pytest.fixture(scope="module")
def pairs(ctx, keys):
    """the two forged pairs; each set is invalid to the oracle"""
    out = {"offset": offset_pair(*single_sets(ctx, keys, "rlc-forge-offs", 2)),
           "swap": swapped_pair(ctx, keys, 900, 901, bd.msg("rlc-forge-swap", 0))}
    for fa, fb in out.values():
        assert oracle_each([fa, fb]) == [0, 0]
    return out


def oracle_each(sets):
    return co.verify_each([p[0] for p, _, _ in sets], [m for _, m, _ in sets], [s for _, _, s in sets])


def expectation(jobs, forged):
    """(per-job verdicts, batch_retries, batch_sigs_success) of the package; `forged`: the forged
    sets (each checked invalid by the oracle in `pairs`), every other set valid"""
    flat = [s for js, _ in jobs for s in js]
    per = [0 if any(s is f for f in forged) else 1 for s in flat]
    assert per.count(0) == len(forged)
    jsets, pos = [], 0
    for js, _ in jobs:
        jsets.append(list(range(pos, pos + len(js))))
        pos += len(js)
    exp, retries, success = co.expected_jobs(jsets, [bool(f & 1) for _, f in jobs], per)
    assert exp == [(0, 0) if any(per[i] == 0 for i in js) else (1, 0) for js in jsets]
    return exp, retries, success


def run(c, jobs, seed):
    got, st = c.verify_jobs(jobs, seed=seed)
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got], st["batch_retries"], st["batch_sigs_success"]


def check(c, jobs, forged, seeds=SEEDS):
    exp = expectation(jobs, forged)
    for seed in seeds:
        got = run(c, jobs, seed)
        bad = [(j, g, e) for j, (g, e) in enumerate(zip(got[0], exp[0])) if g != e]
        assert not bad, (seed, bad[:10])
        assert got[1:] == exp[1:], (seed, got[1:], exp[1:])
    return exp


def names(c):
    return [k for k, _ in c.last_kernel_times()]


@pytest.mark.parametrize("kind", KINDS)
def test_two_one_set_batchable_jobs(ctx, valid, pairs, kind):
    """case 1: the package group holds both, each scaled by its own randomizer"""
    fa, fb = pairs[kind]
    jobs = [([s], B) for s in valid[:6]]
    jobs.insert(2, ([fa], B))
    jobs.insert(5, ([fb], B))
    check(ctx, jobs, (fa, fb))


@pytest.mark.parametrize("kind", KINDS)
def test_both_sets_in_one_job(ctx, valid, pairs, kind):
    """cases 2 and 3: one batchable and one non-batchable two-set job, alone in the package and
    beside valid jobs"""
    fa, fb = pairs[kind]
    for flags in (B, 0):
        check(ctx, [([fa, fb], flags)], (fa, fb))
        check(ctx, [([valid[0]], B), ([fa, fb], flags), ([valid[1]], B), (list(valid[2:4]), 0)], (fa, fb))


@pytest.mark.parametrize("kind", KINDS)
def test_one_set_jobs_in_the_merged_nonbatchable_group(ctx, ab_ctx, valid, pairs, kind, monkeypatch):
    """case 4: one-set non-batchable jobs are verified unscaled when each is a group of its own,
    and must be scaled in the merged group (lsg_plan.hpp plan_groups).  Shipped library and
    one group per job (A/B library, LSG_NB_MERGE=0): identical verdicts and counters."""
    fa, fb = pairs[kind]
    jobs = [([fa], 0), (list(valid[0:2]), 0), ([fb], 0), ([valid[2]], 0)]
    exp = check(ctx, jobs, (fa, fb))
    monkeypatch.setenv("LSG_NB_MERGE", "0")
    assert check(ab_ctx, jobs, (fa, fb)) == exp
    monkeypatch.delenv("LSG_NB_MERGE")
    assert check(ab_ctx, jobs, (fa, fb)) == exp


@pytest.mark.parametrize("kind", KINDS)
def test_two_unscaled_sets_never_share_a_check(ctx, valid, pairs, kind):
    """case 5: the package's only batchable set and a one-set non-batchable job, both r_i = 0"""
    fa, fb = pairs[kind]
    check(ctx, [([fa], B), ([fb], 0)], (fa, fb))
    check(ctx, [([fb], 0), ([fa], B)], (fa, fb))
    # and the valid shape of the same structure stays valid
    check(ctx, [([valid[0]], B), ([valid[1]], 0)], ())


def test_swap_inside_a_message_key_sum(ctx, ab_ctx, keys, monkeypatch):
    """case 6: 6 sets of one message, two of them with each other's signature, and 6 of another
    message: one Miller pair per message (shipped) and one per set (A/B library, LSG_MSG_AGG=0)"""
    sks, pks = keys
    ma, mb = bd.msg("rlc-forge-m", 0), bd.msg("rlc-forge-m", 1)
    sa = ctx.sign(sks[100:106], [ma] * 6)
    sb = ctx.sign(sks[106:112], [mb] * 6)
    sets = [([pks[100 + k]], ma, sa[k]) for k in range(6)] + [([pks[106 + k]], mb, sb[k]) for k in range(6)]
    fa, fb = (sets[1][0], ma, sa[4]), (sets[4][0], ma, sa[1])
    assert oracle_each([fa, fb]) == [0, 0]
    sets[1], sets[4] = fa, fb
    jobs = [([s], B) for s in sets]
    exp = check(ctx, jobs, (fa, fb))
    ctx.verify_jobs(jobs, seed=SEEDS[0])
    assert "k_slp_items_msg" in names(ctx)
    monkeypatch.setenv("LSG_MSG_AGG", "0")
    assert check(ab_ctx, jobs, (fa, fb)) == exp
    ab_ctx.verify_jobs(jobs, seed=SEEDS[0])
    assert "k_slp_items_msg" not in names(ab_ctx)


@pytest.mark.parametrize("kind", KINDS)
def test_pair_in_a_bucket_msm_package(ctx, valid, pairs, kind):
    """case 7: 256 valid one-set jobs and the pair: the package group sums by buckets, the chunk
    and job phases localise the two jobs"""
    fa, fb = pairs[kind]
    jobs = [([s], B) for s in valid[:256]]
    jobs.insert(77, ([fa], B))
    jobs.insert(200, ([fb], B))
    _, retries, _ = check(ctx, jobs, (fa, fb))
    assert retries == 2  # two of the 16 chunks
    ctx.verify_jobs(jobs, seed=SEEDS[0])
    assert "msm_buckets" in names(ctx)


def _coalesced(c, filler, pkgs, seed):
    """the packages submitted while a launch of the filler package is on the device (one launch
    in flight allowed: they are held and go out together); per package (verdicts, counters)"""
    from lodestar_amd._native import PreparedJobs
    pkgs = [PreparedJobs(p) for p in pkgs]
    c.set_coalesce(64, 1)  # (the filler is larger: it launches on its own)
    try:
        t0 = c.submit_jobs(filler, seed=seed)
        tickets = [c.submit_jobs(p, seed=seed) for p in pkgs]
        # the filler still runs after the last submission: every package was held behind it, and
        # the held packages leave as one launch (the case cannot silently become separate launches)
        assert not c.poll(t0), "the filler package finished before the packages were submitted"
        assert all(t is not None and (t[0] >> 8) & 255 == 4 for t in tickets)  # coalesced tickets
        out = []
        for t in reversed(tickets):
            got, st = c.wait_jobs(t)
            out.append(([(g[0], g[1] if g[0] == 2 else 0) for g in got], st["batch_retries"], st["batch_sigs_success"]))
        assert c.wait_jobs(t0)[0] == [(1, 0)] * filler.n_jobs
        return out[::-1]
    finally:
        c.set_coalesce(0, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_pair_in_coalesced_packages(valid, pairs, kind):
    """case 8: (a) three packages in one launch, two of them one lone batchable half each (each
    r_i = 0: its sub-package's group is that set alone) and a valid one; (b) the pair inside one
    sub-package next to a valid sub-package.  Verdicts and counters equal those of separate
    launches and the oracle's."""
    from lodestar_amd._native import Context, PreparedJobs
    fa, fb = pairs[kind]
    c, ref = Context(0), Context(0)
    try:
        filler = PreparedJobs([([s], B) for s in valid[:256]] * 32)  # 8192 sets: on the device for milliseconds
        ok = [([s], B) for s in valid[260:263]]
        for pkgs, forged in (([[([fa], B)], [([fb], B)], ok], ((fa,), (fb,), ())),
                             ([[([fa], B), ([fb], B)], ok], ((fa, fb), ()))):
            exp = [expectation(p, f) for p, f in zip(pkgs, forged)]
            for seed in SEEDS:
                assert _coalesced(c, filler, pkgs, seed) == exp, seed
                assert [run(ref, p, seed) for p in pkgs] == exp, seed
    finally:
        c.close()
        ref.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pair_in_one_miller_item_small(ab_ctx, valid, pairs, kind, monkeypatch):
    """case 9, A/B library with the programs off (four-set Miller items at every size): 40
    one-set jobs, the pair at sets 4 and 5 -- one item of phase C1"""
    fa, fb = pairs[kind]
    monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    sets = list(valid[:40])
    sets[4], sets[5] = fa, fb
    check(ab_ctx, [([s], B) for s in sets], (fa, fb))


@pytest.fixture(scope="module")
def many(ctx, keys):
    return tuple(single_sets(ctx, keys, "rlc-forge-many", 8400))


@pytest.mark.parametrize("kind", KINDS)
def test_pair_in_one_miller_item_large(ctx, many, pairs, kind):
    """case 9, shipped library in the shape of test_gpu_configs.py
    test_thrown_chunk_localises_its_live_jobs: more than 8192 distinct messages and more than
    2048 sets (four-set items, k_miller_fused), the pair at sets 4 k and 4 k + 1"""
    fa, fb = pairs[kind]
    sets = list(many)
    sets[4 * 500], sets[4 * 500 + 1] = fa, fb
    check(ctx, [([s], B) for s in sets], (fa, fb))


@pytest.mark.parametrize("kind", KINDS)
def test_pair_in_a_caller_group(ctx, valid, pairs, kind):
    """case 10: lsg_submit_jobs_grouped: the group's aggregate is the oracle's sum of the three
    valid signatures, its count 3"""
    fa, fb = pairs[kind]
    sets = [valid[10], fa, valid[11], fb, valid[12]]
    jobs = [([s], B) for s in sets]
    exp = expectation(jobs, (fa, fb))
    acc = None
    for s in (valid[10], valid[11], valid[12]):
        acc = E2.add(acc, g2_uncompress(s[2]))
    for seed in SEEDS:
        got, st, aggs = ctx.verify_jobs_grouped(jobs, [0] * 5, 1, seed=seed)
        assert ([(g[0], g[1] if g[0] == 2 else 0) for g in got], st["batch_retries"], st["batch_sigs_success"]) == exp
        assert aggs == [(g2_compress(acc), 3)]


def test_controls(ctx, keys, valid):
    """case 11: a valid set listed twice stays valid (as two jobs and inside one job); an offset
    pair under ONE public key on two messages is rejected"""
    sks, pks = keys
    s = valid[20]
    check(ctx, [([s], B), ([valid[21]], B), ([s], B)], ())
    check(ctx, [([s, s], B)], ())
    check(ctx, [([s, s], 0), ([s], 0)], ())
    ms = [bd.msg("rlc-forge-onekey", k) for k in range(2)]
    sg = ctx.sign([sks[33], sks[33]], ms)
    fa, fb = offset_pair(([pks[33]], ms[0], sg[0]), ([pks[33]], ms[1], sg[1]))
    assert oracle_each([fa, fb]) == [0, 0]
    check(ctx, [([fa], B), ([valid[22]], B), ([fb], B)], (fa, fb))
    check(ctx, [([fa, fb], B)], (fa, fb))
    check(ctx, [([fa, fb], 0)], (fa, fb))
