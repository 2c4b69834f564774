"""The bucket pass of the signature MSM on the device (k_msm_bucket_seg, lsg_k_sig.hip; plan_buckets,
lsg_plan.hpp).  Every test here needs an MI355X.

a) The kernel alone, through lsg_check_msm_buckets: the caller's points, flags, index list and
   chunk triples in, the bucket sums out, compressed (the mixed and the complete additions leave
   other projective representatives).  Three forms on the same input -- the fold with one Fp2
   component per lane, its pair-form twin, and the path it replaces (projective copies by
   k_sig_proj summed by k_seg_reduce<1>) -- against each other and against the oracle's group law,
   per lane-pair count 1, 2, 4, 8 and 32 on buckets of 0, 1, ips - 1, ips, ips + 1, cap and
   cap + 1 members (cap = 64 per lane pair; cap + 1 takes a second pass), the same point twice
   where one lane pair meets both, P then -P then more, buckets whose members are all unusable
   (err, inf and pinf, one kind each), and an unusable member first and last.
b) Whole packages through lsg_submit_jobs with a nonzero seed at 256, 257 and 600 single-key
   sets and one package of two groups of 300: verdicts and counters against the C restatement of
   the oracle, the exported partial byte for byte against the Python oracle under the seeded
   randomizers (its per-set terms computed once for all sizes: the randomizers go by position) and
   against the A/B library with LSG_MSM_FOLD=0; one signature outside G2 and one infinite key
   inside the group; and a failing package of 512 sets in two non-batchable jobs, whose fallback
   groups of 256 run their own bucket MSM."""
import random

import pytest

from oracle import verifier as ov
from oracle.curves import E1, E2, G1_GEN, G2_GEN, BlstError, g2_compress
from oracle.fields import R, f12_coeffs
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co

pytestmark = pytest.mark.gpu
N_KEYS = 64
M64 = (1 << 64) - 1
INF96 = bytes([0xC0]) + bytes(95)
INF_PK = bytes([0x40]) + bytes(95)
FOLD = 64  # members per lane pair of a first-pass chunk (max(SEG_FOLD, SEG_FOLD_WIDE))
SEED = 0x6D736D21


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


def names(c):
    return [k for k, _ in c.last_kernel_times()]


# ---------------------------------------------------------------- a) the kernel alone
# point slots: 0..11 usable, 12 = -slot 0, 13 / 14 / 15 unusable by err / inf / pinf
N_GOOD, NEG0, BAD_ERR, BAD_INF, BAD_PINF = 12, 12, 13, 14, 15


@pytest.fixture(scope="module")
def slots():
    rnd = random.Random(2121)
    pts = [E2.mul(G2_GEN, rnd.randrange(1, R)) for _ in range(N_GOOD)]
    pts.append(E2.neg(pts[0]))
    pts += [E2.mul(G2_GEN, rnd.randrange(1, R)) for _ in range(3)]
    err = [0] * 13 + [3, 0, 0]
    inf = [0] * 14 + [1, 0]
    pinf = [0] * 15 + [1]
    return pts, [g2_compress(p) for p in pts], err, inf, pinf


def bucket_lists(l):
    """the member lists (point slots) of one call at 2^l lane pairs per bucket"""
    rnd = random.Random(77 + l)
    ips, cap = 1 << l, FOLD << l

    def pick(n):
        return [rnd.randrange(N_GOOD) for _ in range(n)]

    def strided(seq):  # lane pair 0 meets members 0, ips, 2 ips, ...
        m = pick(ips * len(seq))
        for k, v in enumerate(seq):
            m[ips * k] = v
        return m

    out = [pick(n) for n in sorted({0, 1, max(ips - 1, 0), ips, ips + 1, cap, cap + 1})]
    out.append(strided([0, 0, 1]))                     # a doubling inside the mixed addition
    out.append(strided([0, NEG0, 1, 1]))               # back to the identity mid-fold, then on
    out.append(strided([0, NEG0]))
    out.append([0, NEG0])                              # opposite partial sums meet in the butterfly (ips >= 2)
    out.append([0] * (ips + 1))                        # equal partial sums meet in the butterfly
    for bad in (BAD_ERR, BAD_INF, BAD_PINF):
        out.append([bad] * (2 * ips + 1))
    out.append(strided([BAD_ERR, 1, 0, BAD_INF]))      # unusable first and last
    out.append([BAD_PINF] + pick(ips) + [BAD_ERR])
    return out, cap


def plan_of(lists, cap):
    """index list, first-pass triples by descending length, second-pass triples, partial sums"""
    idx, first, second, n_tmp = [], [], [], 0
    for b, m in enumerate(lists):
        off = len(idx)
        idx += m
        if len(m) <= cap:
            first.append((off, len(m), b))
        else:
            t0 = n_tmp
            for o in range(0, len(m), cap):
                first.append((off + o, min(cap, len(m) - o), -(n_tmp + 1)))
                n_tmp += 1
            second.append((t0, n_tmp - t0, b))
    first.sort(key=lambda t: -t[1])
    return idx, first, second, n_tmp


def oracle_sum(pts, err, inf, pinf, members):
    count = {}
    for s in members:
        if not (err[s] or inf[s] or pinf[s]):
            count[s] = count.get(s, 0) + 1
    acc = None
    for s, k in count.items():
        acc = E2.add(acc, E2.mul(pts[s], k))
    return INF96 if acc is None else g2_compress(acc)


@pytest.mark.parametrize("l", [0, 1, 2, 3, 5])
def test_bucket_sums_three_forms_and_the_oracle(ctx, slots, l):
    pts, encs, err, inf, pinf = slots
    lists, cap = bucket_lists(l)
    idx, first, second, n_tmp = plan_of(lists, cap)
    assert second and max(t[1] for t in first) == cap  # a full chunk and a second pass are among the cases
    want = [oracle_sum(pts, err, inf, pinf, m) for m in lists]
    assert want.count(INF96) >= 5
    got = {}
    for mode in (0, 1, 2):
        got[mode] = ctx.check_msm_buckets(mode, encs, err, inf, pinf, idx, first, l, len(lists), chunks2=second,
                                          ips_log2_2=0, n_tmp=n_tmp)
        assert "msm_buckets" in names(ctx) and ("k_sig_prep" in names(ctx)) == (mode == 2)
    bad = [(mode, b, len(lists[b])) for mode in got for b in range(len(lists)) if got[mode][b] != want[b]]
    assert not bad, bad[:10]


def test_bucket_hook_refuses_what_the_kernel_would_follow_out_of_bounds(ctx, slots):
    _, encs, err, inf, pinf = slots
    ok = dict(idx=[0, 1, 2], chunks=[(0, 3, 0)], ips_log2=1, n_out=1)
    assert ctx.check_msm_buckets(0, encs, err, inf, pinf, **ok) == ctx.check_msm_buckets(2, encs, err, inf, pinf, **ok)
    for broken in (dict(ok, idx=[0, 1, 16]), dict(ok, chunks=[(1, 3, 0)]), dict(ok, chunks=[(0, 3, 1)]),
                   dict(ok, chunks=[(0, 3, -1)]), dict(ok, ips_log2=6), dict(ok, chunks=[(0, 2, 0), (2, 1, 0)])):
        with pytest.raises(RuntimeError):
            ctx.check_msm_buckets(0, encs, err, inf, pinf, **broken)


# ---------------------------------------------------------------- b) whole packages
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


BAD_SIG, BAD_KEY = 100, 200


@pytest.fixture(scope="module")
def sets600(ctx):
    """600 single-key sets on 600 messages; set 100's signature is on E2 outside G2 and set 200's
    key is pk - pk.  With them the oracle's per-set terms under the seeded randomizers, as
    oracle.verifier.batch_partial forms them: (error code, ML(r pk, H(m)), r sig), computed once."""
    n = 600
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    neg = ctx.sk_to_pk([R - sk for sk in sks])
    msgs = [bd.msg("msm-fold", i) for i in range(n)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
    sets = [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(n)]
    sets[BAD_SIG] = bd.corrupt_not_in_group(sets[BAD_SIG])
    sets[BAD_KEY] = ([pks[BAD_KEY % N_KEYS], neg[BAD_KEY % N_KEYS]], msgs[BAD_KEY], sigs[BAD_KEY])
    flat = [(INF_PK if i == BAD_KEY else sets[i][0][0], sets[i][1], sets[i][2]) for i in range(n)]
    rnd = splitmix(SEED, n)
    terms = []
    for (pkb, m, sigb), r in zip(flat, rnd):
        try:
            sig = ov.signature_from_bytes(sigb, True)
            pk = ov.public_key_from_bytes(pkb)
            if pk is None:
                raise BlstError(6)
        except BlstError as e:
            terms.append((e.code, None, None))
            continue
        terms.append((0, ov.miller_loop_fast(E1.mul(pk, r), ov.hash_to_g2(m)), E2.mul(sig, r)))
    assert [i for i, t in enumerate(terms) if t[0]] == [BAD_SIG, BAD_KEY]
    per_set = co.verify_each([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat])
    assert [i for i, v in enumerate(per_set) if v != 1] == [BAD_SIG, BAD_KEY] and all(v < 0 for v in (per_set[100], per_set[200]))
    return sets, terms, per_set


def oracle_partial(terms, n):
    """oracle.verifier.batch_partial of the first n sets from their terms"""
    gt, S = ov.F12_ONE, None
    for code, f, rs in terms[:n]:
        if code == 0:
            S = E2.add(S, rs)
            gt = ov.f12_mul(gt, f)
    if S is not None:
        gt = ov.f12_mul(gt, ov.f12_conj(ov.miller_loop_fast(G1_GEN, S)))
    return _f12_bytes(gt)


def run_package(c, jobs, monkeypatch=None, **env):
    """-> (partial, has_batch, per-job results, counters, kernel names) under the given A/B switches"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        t = c.submit_jobs(jobs, seed=SEED)
        part, has = c.jobs_partial(t)
        got, stats = c.wait_jobs(t)
        counters = {k: stats[k] for k in ("batch_retries", "batch_sigs_success", "n_final_exps", "key_error", "key_error_job")}
        return part, has, got, counters, names(c)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def expect(jobs, per_set):
    jsets, pos = [], 0
    for sets, _ in jobs:
        jsets.append(list(range(pos, pos + len(sets))))
        pos += len(sets)
    return co.expected_jobs(jsets, [bool(f & 1) for _, f in jobs], per_set)


def check_verdicts(got, stats, jobs, per_set):
    exp, retries, success = expect(jobs, per_set)
    bad = [(j, g, e) for j, (g, e) in enumerate(zip(got, exp)) if (g[0], g[1] if g[0] == 2 else 0) != e]
    assert not bad, bad[:10]
    assert stats["batch_retries"] == retries and stats["batch_sigs_success"] == success, (stats, retries, success)


def packages():
    def singles(n):
        return lambda sets: [([s], 1) for s in sets[:n]]
    return {"256": (singles(256), 256), "257": (singles(257), 257), "600": (singles(600), 600),
            "2x300": (lambda sets: [([s], 1) for s in sets[:300]] + [(sets[300:600], 0)], 300)}


@pytest.mark.parametrize("name", ["256", "257", "600", "2x300"])
def test_packages_against_the_oracle_and_the_present_path(ctx, ab_ctx, sets600, monkeypatch, name):
    sets, terms, per_set = sets600
    make, n_group = packages()[name]
    jobs = make(sets)
    n_sets = sum(len(s) for s, _ in jobs)
    part, has, got, stats, launched = run_package(ctx, jobs)
    assert has and "msm_buckets" in launched and "k_sig_prep" not in launched, launched
    check_verdicts(got, stats, jobs, per_set[:n_sets])
    assert part == oracle_partial(terms, n_group)
    old = run_package(ab_ctx, jobs, monkeypatch, LSG_MSM_FOLD="0")
    assert "msm_buckets" in old[4] and "k_sig_prep" in old[4], old[4]
    assert (part, has, got, stats) == old[:4]
    new = run_package(ab_ctx, jobs, monkeypatch, LSG_MSM_FOLD="1")
    assert "k_sig_prep" not in new[4] and (part, has, got, stats) == new[:4]
    if name == "257":  # the pair-form fold, and more and fewer lane pairs per bucket than the plan takes
        for env in (dict(LSG_FP2_LANES="0"), dict(LSG_MSM_IPS="0"), dict(LSG_MSM_IPS="3"), dict(LSG_MSM_IPS="5")):
            assert (part, has, got, stats) == run_package(ab_ctx, jobs, monkeypatch, **env)[:4], env


def test_failing_package_fallback_groups_run_their_own_buckets(ctx, ab_ctx, sets600, monkeypatch):
    """512 sets in two non-batchable jobs of 256, one set signed over another message: the merged
    group of 512 fails and each job is checked alone, a group of 256 sets on its own bucket MSM"""
    sets, _, _ = sets600
    mine = [s for i, s in enumerate(sets) if i not in (BAD_SIG, BAD_KEY)][:512]
    mine[300] = bd.corrupt_wrong_message(mine[300])
    flat = [(p[0], m, s) for p, m, s in mine]
    per_set = co.verify_each([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat])
    assert [i for i, v in enumerate(per_set) if v != 1] == [300] and per_set[300] == 0
    jobs = [(mine[:256], 0), (mine[256:], 0)]
    part, has, got, stats, launched = run_package(ctx, jobs)
    assert [g[0] for g in got] == [1, 0]
    check_verdicts(got, stats, jobs, per_set)
    # phase A's merged group, then the fallback phase's two groups in one launch: no projective copies
    assert launched.count("msm_buckets") >= 2 and "k_sig_prep" not in launched, launched
    old = run_package(ab_ctx, jobs, monkeypatch, LSG_MSM_FOLD="0")
    assert old[4].count("msm_buckets") >= 2 and "k_sig_prep" in old[4]
    assert (part, has, got, stats) == old[:4]


def test_package_of_4096_sets_on_the_multi_pair_plan(ctx, ab_ctx, monkeypatch):
    """4,096 sets, 16 members per bucket: the shipped library plans several lane pairs per bucket in
    descending order (what the firehose runs).  Verdicts and counters against the C restatement of
    the oracle, everything byte for byte against LSG_MSM_FOLD=0; one signature outside G2 inside"""
    n = 4096
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    msgs = [bd.msg("msm-fold-4k", i) for i in range(n)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
    sets = [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(n)]
    sets[1000] = bd.corrupt_not_in_group(sets[1000])
    per_set = co.verify_each([s[0][0] for s in sets], [s[1] for s in sets], [s[2] for s in sets])
    assert [i for i, v in enumerate(per_set) if v != 1] == [1000] and per_set[1000] < 0
    jobs = [([s], 1) for s in sets]
    part, has, got, stats, launched = run_package(ctx, jobs)
    assert has and "msm_buckets" in launched and "k_sig_prep" not in launched, launched
    check_verdicts(got, stats, jobs, per_set)
    old = run_package(ab_ctx, jobs, monkeypatch, LSG_MSM_FOLD="0")
    assert "k_sig_prep" in old[4]
    assert (part, has, got, stats) == old[:4]
    assert ab_ctx.final_verify([part])
