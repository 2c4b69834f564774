"""LSG_JOB_VALIDATE_KEYS, lsg_deposit_signing_roots and lsg_verify_deposits on the GPU, against
tests/golden/deposits.json (made by the Python oracle, tests/golden/gen_deposits.py), the
Python oracle's KeyValidate and tests/cpu_oracle.py's worker.ts rules.  Every test here needs
an MI355X.

Expected verdicts never come from the GPU.  The good sets are checked valid by the C oracle
once (module fixture); a flagged job's bad key is a per-set error with the oracle's
KeyValidate code (`per_set[i] = -code` in cpu_oracle.expected_jobs); an unflagged job's odd
key gets what the oracle's plain verify says.
"""
import hashlib
import json
import os

import pytest

from oracle import verifier as ov
from oracle.curves import E1, BlstError, g1_compress, g1_deserialize, g1_serialize
from oracle.fields import R
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_KEYS = 64
B, V = 1, 4  # LSG_JOB_BATCHABLE, LSG_JOB_VALIDATE_KEYS


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(ctx):
    """Shared inputs, made once: 192 valid single-key sets over 64 interop keys (signed on the
    GPU, checked valid by the C oracle here), and the odd keys with their oracle codes."""
    sks = [interop_secret_key(i) for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    n = 192
    msgs = [hashlib.sha256(b"lodestar-mi355x" + b"keyvalidate" + i.to_bytes(8, "little")).digest() for i in range(n)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
    sets = [([pks[i % N_KEYS]], msgs[i], sigs[i]) for i in range(n)]
    assert co.verify_each([s[0][0] for s in sets], msgs, sigs) == [1] * n
    T = E1.mul(bd.g1_not_in_group(), R)  # in the cofactor torsion, not O
    assert T is not None

    def alias(i):  # a second byte string for signer i: pk_i + T
        return g1_serialize(E1.add(g1_deserialize(pks[i % N_KEYS]), T))
    off_curve = bytearray(pks[5])
    off_curve[95] ^= 1
    odd = {"alias": alias, "inf": bytes([0x40]) + bytes(95), "off_curve": bytes(off_curve)}
    return {"sks": sks, "pks": pks, "sets": sets, "odd": odd}


def kv_code(pk):
    """the oracle's KeyValidate code of one encoded key (0: valid)"""
    try:
        ov.public_key_validate(pk)
        return 0
    except BlstError as e:
        return e.code


def plain_verify(s):
    """the oracle's verify of one single-key set without KeyValidate (an unflagged job's set)"""
    try:
        return int(ov.verify_single(ov.public_key_from_bytes(s[0][0]), s[1], ov.signature_from_bytes(s[2], True)))
    except BlstError as e:
        return -e.code


def with_key(s, pk):
    return ([pk], s[1], s[2])


def bad_key_for(data, i, kind):
    k = data["odd"][kind]
    return k(i) if callable(k) else k


def mixed_package(data, n):
    """n flagged single-key batchable jobs (sets 0..n-1) with bad keys at flagged positions 0,
    31, 32, 127, 128 and last, interleaved with unflagged good jobs (every third).  Returns
    (jobs, per_set) with per_set in job order."""
    sets = data["sets"]
    kinds = ["alias", "inf", "off_curve"]
    bad_at = sorted({p for p in (0, 31, 32, 127, 128, n - 1) if p < n})
    jobs, per = [], []
    for i in range(n):
        s = sets[i]
        if i in bad_at:
            pk = bad_key_for(data, i, kinds[bad_at.index(i) % 3])
            code = kv_code(pk)
            assert code in (2, 3, 6)
            jobs.append(([with_key(s, pk)], B | V))
            per.append(-code)
        else:
            jobs.append(([s], B | V))
            per.append(1)
        if i % 3 == 0:
            jobs.append(([sets[129 + i // 3]], B))
            per.append(1)
    return jobs, per


def expected(jobs, per):
    jsets, pos = [], 0
    for sets, _ in jobs:
        jsets.append(list(range(pos, pos + len(sets))))
        pos += len(sets)
    return co.expected_jobs(jsets, [bool(f & B) for _, f in jobs], per)


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


def check(got, stats, jobs, per, counters=True):
    exp, retries, success = expected(jobs, per)
    bad = [(j, g, e) for j, (g, e) in enumerate(zip(norm(got), exp)) if g != e]
    assert not bad, bad[:10]
    assert stats["key_error"] == 0, stats
    if counters:
        assert (stats["batch_retries"], stats["batch_sigs_success"]) == (retries, success), (stats, retries, success)


# ---- deposits
def fixture_cases():
    return json.load(open(os.path.join(HERE, "golden", "deposits.json")))["cases"]


def test_deposit_signing_roots_match_fixture(ctx):
    cases = fixture_cases()
    msgs = [bytes.fromhex(c["data"])[:88] for c in cases]
    dom = bytes.fromhex(cases[0]["domain"])
    want = [bytes.fromhex(c["root"]) for c in cases]
    assert ctx.deposit_signing_roots(msgs, dom) == want
    assert ctx.deposit_signing_roots(msgs, [dom] * len(msgs)) == want  # one domain per object
    assert ctx.deposit_signing_roots(msgs[:1], dom) == want[:1]


def test_verify_deposits_reproduces_fixture(ctx):
    cases = fixture_cases()
    dom = bytes.fromhex(cases[0]["domain"])
    datas = [bytes.fromhex(c["data"]) for c in cases]
    want = [(c["valid"], c["err"]) for c in cases]
    assert ctx.verify_deposits(datas[:1], dom, seed=5) == [(1, 0)]  # the genesis KAT alone
    assert ctx.verify_deposits(datas, dom, seed=5) == want
    assert ctx.verify_deposits(datas, dom) == want  # OS randomizers
    # each deposit alone: a lone set is verified unscaled, and a lone bad key has no group at all
    for d, w in zip(datas, want):
        assert ctx.verify_deposits([d], dom) == [w]
    # order and neighbours do not matter: reversed, and each bad deposit between two KATs
    assert ctx.verify_deposits(datas[::-1], dom, seed=6) == want[::-1]
    tri = [d for x in datas[1:] for d in (datas[0], x, datas[0])]
    assert ctx.verify_deposits(tri, dom, seed=7) == [v for w in want[1:] for v in (want[0], w, want[0])]


def test_verify_deposits_across_packages(ctx, data):
    """n above one package (8,192 deposits): the verdicts come back in order from several
    pipeline slots; bad deposits at the package bounds."""
    from oracle import interop as oi
    n = 8192 + 37
    dom = oi.compute_domain(oi.DOMAIN_DEPOSIT, bytes.fromhex("00000000"), bytes(32))
    pk48 = [g1_compress(g1_deserialize(p)) for p in data["pks"]]
    wc = [hashlib.sha256(p).digest() for p in pk48]
    msgs = [pk48[i % N_KEYS] + wc[i % N_KEYS] + (32 * 10 ** 9 + i).to_bytes(8, "little") for i in range(n)]
    roots = [oi.compute_signing_root(oi.deposit_message_root(m[:48], m[48:80], int.from_bytes(m[80:], "little")), dom)
             for m in msgs]
    assert ctx.deposit_signing_roots(msgs, dom) == roots
    sigs = ctx.sign([data["sks"][i % N_KEYS] for i in range(n)], roots)
    assert co.verify_each([data["pks"][i % N_KEYS] for i in range(n)], roots, sigs) == [1] * n
    deps = [m + s for m, s in zip(msgs, sigs)]
    want = [(1, 0)] * n
    for i in (0, 8191, 8192, n - 1):  # another deposit's signature: validates, does not verify
        deps[i] = msgs[i] + sigs[i + 1 if i + 1 < n else 0]
        want[i] = (0, 0)
    alias48 = g1_compress(g1_deserialize(data["odd"]["alias"](3)))
    for i in (1, 8190, 8193):  # an alias key (its root differs: the signature is then beside the point)
        deps[i] = alias48 + deps[i][48:]
        want[i] = (0, 3)
    assert kv_code(alias48) == 3
    assert ctx.verify_deposits(deps, dom, seed=9) == want
    # more packages than the call keeps outstanding (four): the oldest is waited on to go on
    assert ctx.verify_deposits(deps * 5, dom, seed=10) == want * 5


# ---- the job flag
@pytest.mark.parametrize("n", [1, 33, 129])
def test_flagged_jobs_shapes(ctx, data, n):
    jobs, per = mixed_package(data, n)
    got, stats = ctx.verify_jobs(jobs, seed=11)
    check(got, stats, jobs, per)
    assert any(g[0] == 2 for g in got) and (n == 1 or any(g[0] == 1 for g in got))


def test_alias_and_infinity_before_and_after(ctx, data):
    """The same set in an unflagged and in a flagged job of one package: unflagged, the
    oracle's plain verify decides (the alias key verifies: the pairing cannot see T); flagged,
    KeyValidate rejects it."""
    sets = data["sets"]
    alias = with_key(sets[0], data["odd"]["alias"](0))
    inf = ([data["odd"]["inf"]], sets[1][1], bd.corrupt_infinity(sets[1])[2])
    pv_alias, pv_inf = plain_verify(alias), plain_verify(inf)
    assert kv_code(alias[0][0]) == 3 and kv_code(inf[0][0]) == 6
    jobs = [([alias], B), ([alias], B | V), ([inf], B), ([inf], B | V)] + [([s], B) for s in sets[2:8]]
    per = [pv_alias, -3, pv_inf, -6] + [1] * 6
    got, stats = ctx.verify_jobs(jobs, seed=3)
    check(got, stats, jobs, per)
    assert norm(got)[1] == (2, 3) and norm(got)[3] == (2, 6)
    assert norm(got)[0] == ((1, 0) if pv_alias == 1 else (0, 0) if pv_alias == 0 else (2, -pv_alias))
    # non-batchable jobs take the same stage
    jobs = [([alias], 0), ([alias], V), ([inf], V), ([sets[2]], V)]
    got, stats = ctx.verify_jobs(jobs, seed=3)
    check(got, stats, jobs, [pv_alias, -3, -6, 1])


def test_bad_key_is_job_local_when_flagged(ctx, data):
    sets = data["sets"]
    base = [([s], B | (V if i % 2 else 0)) for i, s in enumerate(sets[:40])]
    base[7] = ([bd.corrupt_wrong_message(sets[7])], B)  # an invalid set among them
    per = [1] * 40
    per[7] = 0
    bad = with_key(sets[20], data["odd"]["off_curve"])
    code = kv_code(bad[0][0])
    assert code == 2
    without, st0 = ctx.verify_jobs(base, seed=13)
    check(without, st0, base, per)
    jobs = base[:20] + [([bad], B | V)] + base[20:]
    got, st = ctx.verify_jobs(jobs, seed=13)
    check(got, st, jobs, per[:20] + [-code] + per[20:])
    assert norm(got[:20] + got[21:]) == norm(without) and norm(got)[20] == (2, code)
    # the same key in an unflagged job still rejects the package (worker.ts:41-43)
    jobs[20] = ([bad], B)
    got, st = ctx.verify_jobs(jobs, seed=13)
    assert norm(got) == [(2, code)] * len(jobs) and st["key_error"] == code and st["key_error_job"] == 20


def test_flagged_aggregate_set_first_bad_key_decides(ctx, data):
    sks, pks, sets = data["sks"], data["pks"], data["sets"]
    m = sets[0][1]
    sig = ctx.sign([sum(sks[k] for k in (1, 2, 3)) % R], [m])[0]
    good = ([pks[1], pks[2], pks[3]], m, sig)
    assert co.verify_each([g1_serialize(ov.aggregate_pubkeys([g1_deserialize(p) for p in good[0]]))], [m], [sig]) == [1]
    alias2 = data["odd"]["alias"](2)
    cases = [
        (([pks[1], alias2, data["odd"]["off_curve"]], m, sig), 3),  # second key bad, third worse
        (([pks[1], data["odd"]["inf"], alias2], m, sig), 6),
        (([pks[1], pks[2], data["odd"]["off_curve"]], m, sig), 2),
    ]
    for s, code in cases:
        assert next(c for c in map(kv_code, s[0]) if c) == code
    jobs = [([good], V), ([good], B | V)] + [([s], V) for s, _ in cases] + [([s], B | V) for s, _ in cases]
    per = [1, 1] + [-c for _, c in cases] * 2
    # (job order = staging order here only for the expectation: expected_jobs works per job)
    got, stats = ctx.verify_jobs(jobs, seed=17)
    check(got, stats, jobs, per)
    # key error beats signature error inside a set; the first set in order decides inside a job
    badsig = bd.corrupt_truncate(sets[4])
    both = with_key(badsig, data["odd"]["alias"](4))
    sig_code = -co.verify_each([sets[4][0][0]], [badsig[1]], [badsig[2]])[0]
    assert sig_code == 10
    got, stats = ctx.verify_jobs([([both], V), ([badsig, both], V), ([both, badsig], V), ([badsig], V)], seed=19)
    assert norm(got) == [(2, 3), (2, sig_code), (2, 3), (2, sig_code)] and stats["key_error"] == 0


def test_flag_leaves_index_keys_alone(data):
    from lodestar_amd._native import Context, PkIndices
    c = Context(0)
    try:
        assert c.pubkey_table_set(0, data["pks"][:8]) == [0] * 8
        sets = data["sets"]
        jobs = [([(PkIndices([i]), sets[i][1], sets[i][2])], B | V) for i in range(8)]
        jobs.append(([(PkIndices([1]), sets[0][1], sets[0][2])], V))  # wrong signer: invalid, no error
        jobs.append(([with_key(sets[9], data["odd"]["alias"](9))], B | V))  # byte keys are still validated
        got, stats = c.verify_jobs(jobs, seed=23)
        unflagged, _ = c.verify_jobs([(s, f & ~V) for s, f in jobs[:9]], seed=23)
        assert norm(got)[:9] == norm(unflagged) == [(1, 0)] * 8 + [(0, 0)]
        assert norm(got)[9] == (2, 3) and stats["key_error"] == 0
    finally:
        c.close()


# ---- every path that takes jobs
def test_mixed_package_coalesced(data):
    from lodestar_amd._native import Context
    jobs, per = mixed_package(data, 33)
    c = Context(0)
    try:
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        small = [([s], B) for s in data["sets"][140:150]]
        tickets = [c.submit_jobs(p, seed=29) for p in (small, jobs, small, jobs)]
        assert all(t is not None and t[0] >> 8 & 255 == 4 for t in tickets)  # coalesced tickets
        res = [c.wait_jobs(t) for t in tickets]
        for k in (1, 3):
            check(res[k][0], res[k][1], jobs, per)
        for k in (0, 2):
            assert res[k][0] == [(1, 0)] * 10
    finally:
        c.close()


def test_mixed_package_multi_device_duplicate_ids(ctx, data):
    from lodestar_amd._native import Context
    jobs, per = mixed_package(data, 33)
    c2 = Context(devices=[0, 0])
    try:
        assert c2.device_count() == 2
        got, stats = c2.verify_jobs(jobs, seed=31)
        check(got, stats, jobs, per, counters=False)
        assert norm(got) == norm(ctx.verify_jobs(jobs, seed=31)[0])
        # the 16-job chunks are formed per device: the counters are the sum over the devices'
        # shares (whole jobs by cumulative set count, lsg_assign_jobs) of worker.ts's per share
        from lodestar_amd._native import assign_jobs
        owner = assign_jobs([len(sets) for sets, _ in jobs], 2)
        assert set(owner) == {0, 1}
        retries = success = 0
        for d in (0, 1):
            share = [j for j in range(len(jobs)) if owner[j] == d]
            _, r, k = expected([jobs[j] for j in share], [per[j] for j in share])  # (single-set jobs)
            retries, success = retries + r, success + k
        assert (stats["batch_retries"], stats["batch_sigs_success"]) == (retries, success), (stats, retries, success)
        cases = fixture_cases()
        dom = bytes.fromhex(cases[0]["domain"])
        assert c2.verify_deposits([bytes.fromhex(c["data"]) for c in cases], dom, seed=5) == \
            [(c["valid"], c["err"]) for c in cases]
    finally:
        c2.close()


def test_mixed_package_node_protocol(ctx, data):
    jobs, per = mixed_package(data, 33)
    t = ctx.submit_jobs(jobs, seed=37)
    part, has = ctx.jobs_partial(t)
    # the erroring sets stay out of the package group: the rest of it is valid
    assert has and ctx.final_verify([part])
    got, stats = ctx.wait_jobs_node(t, 1)
    check(got, stats, jobs, per)
    t = ctx.submit_jobs(jobs, seed=37)
    ctx.jobs_partial(t)
    got, stats = ctx.wait_jobs_node(t, 0)  # a failed node check: this GPU's own check decides
    check(got, stats, jobs, per)


# ---- no cost when unused
def test_unflagged_package_launches_no_validation_stage(ctx, data):
    sets = data["sets"]
    ctx.verify_jobs([([s], B) for s in sets[:40]], seed=41)
    names = [k for k, _ in ctx.last_kernel_times()]
    assert names and not [k for k in names if "keyvalidate" in k], names
    ctx.verify_jobs([([s], B | V) for s in sets[:40]], seed=41)
    names = [k for k, _ in ctx.last_kernel_times()]
    assert "k_pk_keyvalidate" in names and "k_pk_keyvalidate_apply" in names, names
    # a flagged job of index keys only has no key to validate
    from lodestar_amd._native import Context, PkIndices
    c = Context(0)
    try:
        c.pubkey_table_set(0, data["pks"][:4])
        c.verify_jobs([([(PkIndices([i]), sets[i][1], sets[i][2])], B | V) for i in range(4)], seed=41)
        names = [k for k, _ in c.last_kernel_times()]
        assert names and not [k for k in names if "keyvalidate" in k], names
    finally:
        c.close()


def test_flagged_submissions_allocate_nothing_after_reserve(ctx, data, capfd, monkeypatch):
    from lodestar_amd._native import PreparedJobs
    sets = data["sets"]
    jobs = [([s], B | V) for s in sets]  # (distinct messages: the plain per-set path, as the firehose)
    jobs[100] = ([with_key(sets[100], data["odd"]["alias"](100))], B | V)
    pj = PreparedJobs(jobs)
    ctx.reserve(4096, n_slots=0)
    monkeypatch.setenv("LSG_TRACE_ALLOC", "1")
    capfd.readouterr()
    before = ctx.allocation_count()
    for rep in range(2):
        tickets = [ctx.submit_jobs(pj) for _ in range(4)]
        for t in tickets:
            res, stats = ctx.wait_jobs(t)
            assert norm(res) == [(2, 3) if j == 100 else (1, 0) for j in range(len(jobs))]
    trace = [ln for ln in capfd.readouterr().err.splitlines() if "lsg alloc" in ln]
    assert ctx.allocation_count() == before, trace


# ---- Node
def test_node_deposits_and_validate_on_gpu(data, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: verifyDeposits over the fixture
    and a flagged verifySignatureSets that rejects the alias key."""
    import shutil
    import subprocess
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    addon = os.path.join(HERE, "..", "lodestar_amd", "napi", "lsg_napi.node")
    assert os.path.exists(addon), "N-API addon not built"
    s = data["sets"][0]
    alias = with_key(s, data["odd"]["alias"](0))
    cases = {
        "good": {"pk": s[0][0].hex(), "msg": s[1].hex(), "sig": s[2].hex()},
        "alias": {"pk": alias[0][0].hex(), "msg": alias[1].hex(), "sig": alias[2].hex()},
        "alias_unvalidated": plain_verify(alias) == 1,
        "keys": {"pks": (s[0][0] + alias[0][0] + data["odd"]["inf"]).hex(),
                 "err": [kv_code(s[0][0]), kv_code(alias[0][0]), kv_code(data["odd"]["inf"])]},
    }
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_deposits_gpu.js"), str(f)], capture_output=True,
                       text=True, timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "deposits gpu ok" in r.stdout, r.stdout + r.stderr
