"""Sets whose message is an SSZ object + domain on the GPU (LSG_MSG_OBJECT):
the signing root is computed by k_msg_roots as the package's first stage.  Expected roots come
from oracle/interop.py (tests/msgobjects.py), expected verdicts from tests/cpu_oracle.py's
worker.ts rules over those roots; every object-form package is also compared with the same
package in root form under the same seed.  Every comparison is exact.  Every test here needs
an MI355X.

Keys are the 64 interop keys; signatures are made with ctx.sign over the oracle's roots."""
import hashlib
import random

import pytest

from oracle import verifier as ov
from oracle.curves import g1_serialize
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import msgobjects as mo

pytestmark = pytest.mark.gpu
B, V = 1, 4  # LSG_JOB_BATCHABLE, LSG_JOB_VALIDATE_KEYS
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job")
PLAIN32, PLAIN45 = "plain32", "plain45"


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    sks = [interop_secret_key(i) for i in range(64)]
    return sks, ctx.sk_to_pk(sks)


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


# ---- 1. roots
def test_roots_of_every_kind(ctx):
    rng = random.Random(41)
    for n_obj in mo.KINDS:
        for n in (1, 63, 64, 65):  # the 64-thread workgroup edge
            objs = [rng.randbytes(n_obj) for _ in range(n)]
            doms = [rng.randbytes(32) for _ in range(n)]
            assert ctx.object_signing_roots(objs, doms) == [mo.signing_root(o, d) for o, d in zip(objs, doms)], (n_obj, n)
            assert "k_object_signing_root" in names(ctx)
            one = ctx.object_signing_roots(objs, doms[0])
            assert one == [mo.signing_root(o, doms[0]) for o in objs], (n_obj, n)
            for size, fn in ((32, ctx.signing_roots), (128, ctx.attestation_signing_roots), (88, ctx.deposit_signing_roots)):
                if size == n_obj:  # byte-equal to the kind's own call
                    assert fn(objs, doms) == ctx.object_signing_roots(objs, doms) and fn(objs, doms[0]) == one
    obj, dom, root = mo.genesis_kat()
    assert ctx.object_signing_roots([obj], dom) == [root] == ctx.deposit_signing_roots([obj], dom)
    with pytest.raises(RuntimeError):
        ctx.object_signing_roots([bytes(33)], dom)
    assert ctx.object_signing_roots([obj], dom) == [root]  # the context stays usable


# ---- 2. equivalence
class Package:
    """n signed sets over messages of the given forms (an object kind's length, PLAIN32 or
    PLAIN45), in object form and in root form; jobs as (first set, count, flags)."""

    def __init__(self, ctx, keys, tag, forms, shape, wrong=(), undecodable=()):
        from lodestar_amd._native import MsgObject
        sks, pks = keys
        rng = random.Random(hashlib.sha256(tag.encode()).digest())
        n = len(forms)
        self.pks = [pks[(3 * i + 1) % 64] for i in range(n)]
        sk = [sks[(3 * i + 1) % 64] for i in range(n)]
        self.obj_msg, self.msg = [], []  # the message in object form; the bytes that are signed
        for f in forms:
            if f == PLAIN32 or f == PLAIN45:
                m = rng.randbytes(32 if f == PLAIN32 else 45)
                self.obj_msg.append(m)
                self.msg.append(m)
            else:
                obj, dom = rng.randbytes(f), rng.randbytes(32)
                self.obj_msg.append(MsgObject(obj, dom))
                self.msg.append(mo.signing_root(obj, dom))
        signed = [hashlib.sha256(m).digest() if i in wrong else m for i, m in enumerate(self.msg)]
        self.sigs = [None] * n
        for length in (32, 45):  # ctx.sign takes messages of one length
            idx = [i for i in range(n) if len(signed[i]) == length]
            for i, s in zip(idx, ctx.sign([sk[i] for i in idx], [signed[i] for i in idx])):
                self.sigs[i] = s
        for i in undecodable:
            self.sigs[i] = bd.corrupt_flip_x_bit((None, None, self.sigs[i]))[2]
        # per-set outcomes: the C oracle over the 32-byte roots, the Python oracle for the rest
        i32 = [i for i in range(n) if len(self.msg[i]) == 32]
        self.per_set = [None] * n
        for i, v in zip(i32, co.verify_each([self.pks[i] for i in i32], [self.msg[i] for i in i32], [self.sigs[i] for i in i32])):
            self.per_set[i] = v
        for i in range(n):
            if self.per_set[i] is None:
                ok = ov.verify_single(ov.public_key_from_bytes(self.pks[i]), self.msg[i], ov.signature_from_bytes(self.sigs[i]))
                self.per_set[i] = 1 if ok else 0
        assert [i for i, v in enumerate(self.per_set) if v == 0] == sorted(wrong), self.per_set
        assert [i for i, v in enumerate(self.per_set) if v < 0] == sorted(undecodable), self.per_set
        self.shape = shape
        assert sum(c for _, c, _ in shape) == n
        self.exp, self.retries, self.success = co.expected_jobs(
            [list(range(p, p + c)) for p, c, _ in shape], [bool(f & B) for _, _, f in shape], self.per_set)

    def sets(self, form):
        msgs = self.obj_msg if form == "object" else self.msg
        return [([pk], m, s) for pk, m, s in zip(self.pks, msgs, self.sigs)]

    def jobs(self, form, shape=None):
        flat = self.sets(form)
        return [(flat[p:p + c], f) for p, c, f in (shape or self.shape)]

    def good(self):
        return [i for i, v in enumerate(self.per_set) if v == 1]


def shape_of(n):
    """jobs of 1-2 sets, every fifth one not batchable"""
    shape, pos = [], 0
    while pos < n:
        cnt = min(1 + len(shape) % 2, n - pos)
        shape.append((pos, cnt, B if len(shape) % 5 != 3 else 0))
        pos += cnt
    return shape


@pytest.fixture(scope="module")
def pkg7(ctx, keys):
    forms = [8, 16, 76, 112, 128, PLAIN32, PLAIN45]
    return Package(ctx, keys, "seven", forms, [(0, 2, B), (2, 1, B), (3, 2, 0), (5, 1, B), (6, 1, 0)], wrong=[2], undecodable=[5])


@pytest.fixture(scope="module")
def pkg65(ctx, keys):
    forms = [(list(mo.KINDS) + [PLAIN32])[i % 8] for i in range(65)]
    forms[20] = PLAIN45
    p = Package(ctx, keys, "sixty-five", forms, shape_of(65), wrong=[10], undecodable=[40])
    assert sum(1 for _, _, f in p.shape if f & B) >= 32 and p.retries >= 1  # chunks, and a fallback
    return p


def check_both_forms(c, pkg, seed, counters=True):
    got_o, st_o = c.verify_jobs(pkg.jobs("object"), seed=seed)
    assert "k_msg_roots" in names(c)
    got_r, st_r = c.verify_jobs(pkg.jobs("root"), seed=seed)
    assert "k_msg_roots" not in names(c)
    assert norm(got_o) == pkg.exp, (norm(got_o), pkg.exp)
    assert got_o == got_r
    assert [st_o[k] for k in COUNTERS] == [st_r[k] for k in COUNTERS]
    if counters:
        assert (st_o["batch_retries"], st_o["batch_sigs_success"], st_o["key_error"]) == (pkg.retries, pkg.success, 0), st_o


def test_lone_sets_of_every_kind(ctx, keys):
    """packages of one set: the lone, unscaled path"""
    for k, form in enumerate(mo.KINDS):
        for flags in (B, 0):
            good = Package(ctx, keys, f"lone{form}", [form], [(0, 1, flags)])
            check_both_forms(ctx, good, seed=11 + k)
            assert good.exp == [(1, 0)]
            assert ctx.verify_sets(good.sets("object"), seed=5) == ctx.verify_sets(good.sets("root"), seed=5) == (1, 0)
        forged = Package(ctx, keys, f"lone-forged{form}", [form], [(0, 1, B)], wrong=[0])
        check_both_forms(ctx, forged, seed=21 + k)
        assert forged.exp == [(0, 0)]


@pytest.mark.parametrize("which", ["pkg7", "pkg65"])
def test_mixed_packages_match_oracle_and_root_form(ctx, which, request):
    pkg = request.getfixturevalue(which)
    check_both_forms(ctx, pkg, seed=3)
    # lsg_batch_partial: byte-equal partials, with the failing sets and without
    for idx in (list(range(len(pkg.msg))), pkg.good()):
        so, sr = pkg.sets("object"), pkg.sets("root")
        part_o, errs_o, any_o = ctx.batch_partial([so[i] for i in idx], seed=8)
        assert "k_msg_roots" in names(ctx)
        part_r, errs_r, any_r = ctx.batch_partial([sr[i] for i in idx], seed=8)
        assert (part_o, errs_o, any_o) == (part_r, errs_r, any_r)
        assert errs_o == [max(0, -pkg.per_set[i]) for i in idx]
        assert ctx.final_verify([part_o]) == all(pkg.per_set[i] == 1 for i in idx if pkg.per_set[i] >= 0)
    # lsg_verify_sets (one maybeBatch call): all good, one forged, one that does not decode
    good = pkg.good()[:6]
    for idx in (good, good + [i for i, v in enumerate(pkg.per_set) if v == 0], good + [i for i, v in enumerate(pkg.per_set) if v < 0]):
        so, sr = pkg.sets("object"), pkg.sets("root")
        got = ctx.verify_sets([so[i] for i in idx], seed=9)
        assert got == ctx.verify_sets([sr[i] for i in idx], seed=9)
        bad = [pkg.per_set[i] for i in idx if pkg.per_set[i] != 1]
        assert got == ((1, 0) if not bad else ((2, -bad[0]) if bad[0] < 0 else (0, 0)))


# ---- 3. dedup
def test_sets_sharing_an_object_share_its_root(ctx, keys):
    from lodestar_amd._native import MsgObject
    sks, pks = keys
    rng = random.Random(77)
    pairs = [(rng.randbytes(128), rng.randbytes(32)), (rng.randbytes(128), rng.randbytes(32)), (rng.randbytes(16), rng.randbytes(32))]
    pairs[1] = (pairs[0][0], pairs[1][1])  # the same object under another domain: another message
    roots = [mo.signing_root(o, d) for o, d in pairs]
    assert len(set(roots)) == 3
    which = [i % 3 for i in range(40)]
    sigs = ctx.sign(sks[:41], [roots[w] for w in which] + [roots[1]])
    sigs[17] = ctx.sign([sks[17]], [roots[(which[17] + 1) % 3]])[0]  # forged: signed over another of the roots
    sets = [([pks[i]], MsgObject(*pairs[which[i]]), sigs[i]) for i in range(40)]
    sets.append(([pks[40]], roots[1], sigs[40]))  # a plain message that equals an object's root
    per_set = co.verify_each(pks[:41], [roots[w] for w in which] + [roots[1]], sigs)
    assert [i for i, v in enumerate(per_set) if v != 1] == [17]
    jobs = [([s], B) for s in sets]
    exp, retries, success = co.expected_jobs([[i] for i in range(41)], [True] * 41, per_set)
    got, stats = ctx.verify_jobs(jobs, seed=13)
    assert norm(got) == exp and exp.count((0, 0)) == 1
    assert (stats["batch_retries"], stats["batch_sigs_success"]) == (retries, success)
    t = dict(ctx.last_kernel_times())
    assert "k_msg_roots" in t and "k_h2c_gather" in t  # four staged messages for 41 sets
    good = [s for i, s in enumerate(sets) if i != 17]
    part, errs, anyerr = ctx.batch_partial(good, seed=2)
    assert not anyerr and ctx.final_verify([part])


# ---- 4. block shape
def test_block_attestations_by_committee_bits_and_object(keys):
    from lodestar_amd._native import Context, MsgObject, PkBits, PkIndices
    from oracle.fields import R
    sks, pks = keys
    c = Context(0)
    try:
        assert c.pubkey_table_set(0, pks) == [0] * 64
        rng = random.Random(19)
        committees = [[rng.randrange(64) for _ in range(n)] for n in (5, 33, 64, 130)]
        assert c.committees_set(0, committees) == [0] * 4
        domain = rng.randbytes(32)
        sets_o, sets_r, agg, roots, sigs = [], [], [], [], []
        for k, rows in enumerate(committees):
            bits = [1 if rng.random() < 0.9 else 0 for _ in rows]
            bits[0] = 1
            raw = bytearray((len(bits) + 7) // 8)
            for j, b in enumerate(bits):
                raw[j >> 3] |= b << (j & 7)
            part = [r for r, b in zip(rows, bits) if b]
            data = rng.randbytes(128)  # AttestationData bytes
            root = mo.signing_root(data, domain)
            sig = c.sign([sum(sks[r] for r in part) % R], [root])[0]
            sets_o.append((PkBits(k, bytes(raw), len(bits)), MsgObject(data, domain), sig))
            sets_r.append((PkIndices(part), root, sig))
            agg.append(g1_serialize(ov.aggregate_pubkeys([ov.public_key_from_bytes(pks[r]) for r in part])))
            roots.append(root)
            sigs.append(sig)
        assert co.verify_each(agg, roots, sigs) == [1] * 4
        got_o, st_o = c.verify_jobs([(sets_o, B)], seed=23)
        assert "k_msg_roots" in names(c) and "k_pk_agg_bits" in names(c)
        got_r, st_r = c.verify_jobs([(sets_r, B)], seed=23)
        assert norm(got_o) == norm(got_r) == [(1, 0)]
        assert [st_o[k] for k in COUNTERS] == [st_r[k] for k in COUNTERS]
        forged = list(sets_o)
        forged[2] = (forged[2][0], MsgObject(rng.randbytes(128), domain), forged[2][2])
        assert norm(c.verify_jobs([(forged, B)], seed=23)[0]) == [(0, 0)]
    finally:
        c.close()


# ---- 5. flagged jobs
def test_validate_keys_job_with_a_bls_change_object(ctx, keys):
    from lodestar_amd._native import MsgObject
    from oracle.curves import E1
    from oracle.fields import R
    sks, pks = keys
    rng = random.Random(31)
    change, domain = rng.randbytes(76), rng.randbytes(32)  # BLSToExecutionChange bytes
    root = mo.signing_root(change, domain)
    sig = ctx.sign([sks[9]], [root])[0]
    assert co.verify_each([pks[9]], [root], [sig]) == [1]
    torsion = g1_serialize(E1.mul(bd.g1_not_in_group(), R))  # in the cofactor torsion, not O
    assert ctx.pubkey_validate([torsion])[0][1] == 3  # BLST_POINT_NOT_IN_GROUP
    for msg in (MsgObject(change, domain), root):
        got, stats = ctx.verify_jobs([([([pks[9]], msg, sig)], B | V), ([([torsion], msg, sig)], B | V)], seed=29)
        assert norm(got) == [(1, 0), (2, 3)] and stats["key_error"] == 0
        assert ("k_msg_roots" in names(ctx)) == isinstance(msg, MsgObject) and "k_pk_keyvalidate" in names(ctx)


# ---- 6. coalesced and multi-device
def test_coalesced_packages(pkg7):
    from lodestar_amd._native import Context
    c = Context(0)
    try:
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        parts = [pkg7.shape[0:2], pkg7.shape[2:3], pkg7.shape[3:5]]
        tickets = [c.submit_jobs(pkg7.jobs("object", sh), seed=29) for sh in parts]
        assert all(t is not None and t[0] >> 8 & 255 == 4 for t in tickets)  # coalesced tickets
        got = [g for t in tickets for g in c.wait_jobs(t)[0]]
        assert norm(got) == pkg7.exp
        tickets = [c.submit_jobs(pkg7.jobs("root", sh), seed=29) for sh in parts]
        assert got == [g for t in tickets for g in c.wait_jobs(t)[0]]
    finally:
        c.close()


def test_multi_device_duplicate_ids(pkg7):
    from lodestar_amd._native import Context
    c = Context(devices=[0, 0])
    try:
        assert c.device_count() == 2
        got, stats = c.verify_jobs(pkg7.jobs("object"), seed=31)
        assert norm(got) == pkg7.exp and stats["key_error"] == 0
        assert got == c.verify_jobs(pkg7.jobs("root"), seed=31)[0]
    finally:
        c.close()


def test_node_protocol(ctx, pkg7):
    good = [(sets, f) for (sets, f), e in zip(pkg7.jobs("object"), pkg7.exp) if e == (1, 0)]
    t = ctx.submit_jobs(good, seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and ctx.final_verify([part])
    assert norm(ctx.wait_jobs_node(t, 1)[0]) == [(1, 0)] * len(good)
    t = ctx.submit_jobs(pkg7.jobs("object"), seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and not ctx.final_verify([part])
    assert norm(ctx.wait_jobs_node(t, 0)[0]) == pkg7.exp


# ---- 7. arguments
def test_argument_errors_leave_the_context_usable(ctx, keys, pkg7):
    from lodestar_amd._native import LSG_ERR_INVALID_ARG, LsgJob, LsgJobResult, MsgObject, PreparedJobs, SetBuffer
    import ctypes
    sks, pks = keys
    good = pkg7.sets("object")[0]
    for bad_msg in (MsgObject(bytes(33), bytes(32)), MsgObject(b"", b"")):  # payload 65; a NULL message
        bad = (good[0], bad_msg, good[2])
        p = PreparedJobs([([good], B), ([good, bad], 0)])
        t = ctypes.c_uint64()
        assert ctx.lib.lsg_submit_jobs(ctx.h, p.jobs, p.n_jobs, 1, ctypes.byref(t)) == LSG_ERR_INVALID_ARG
        for call in (lambda: ctx.verify_jobs([([bad], B)]), lambda: ctx.verify_sets([good, bad]), lambda: ctx.batch_partial([bad, good])):
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                call()
        b = SetBuffer([bad])
        assert (b.arr[0].msg_len & 0x7fffffff, bool(b.arr[0].msg)) == ((65, True) if len(bad_msg) else (0, False))
        check_both_forms(ctx, pkg7, seed=43)  # the next good package is verified correctly
    # a marked length that does name a kind (a Root: 64) with msg == NULL, through the entry points
    for flags in (B, 0):
        b = SetBuffer([good, good])
        b.arr[1].msg, b.arr[1].msg_len = None, 0x80000000 | 64
        job = LsgJob(b.arr, 2, flags)
        t, res, out, errs, anyerr = ctypes.c_uint64(), LsgJobResult(), ctypes.create_string_buffer(576), (ctypes.c_int32 * 2)(), ctypes.c_int32()
        assert ctx.lib.lsg_submit_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(t)) == LSG_ERR_INVALID_ARG
        assert ctx.lib.lsg_verify_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(res), None) == LSG_ERR_INVALID_ARG
        assert ctx.lib.lsg_verify_sets(ctx.h, b.arr, 2, 1, ctypes.byref(res)) == LSG_ERR_INVALID_ARG
        assert ctx.lib.lsg_batch_partial(ctx.h, b.arr, 2, 1, out, errs, ctypes.byref(anyerr)) == LSG_ERR_INVALID_ARG
    check_both_forms(ctx, pkg7, seed=47)
    with pytest.raises(RuntimeError, match=r"\(1\)"):
        ctx._check(ctx.lib.lsg_sign(ctx.h, int(sks[0]).to_bytes(32, "big"), bytes(64), 0x80000000 | 64, 1,
                                    ctypes.create_string_buffer(96)), "lsg_sign")
    with pytest.raises(RuntimeError, match=r"\(1\)"):
        ctx._check(ctx.lib.lsg_hash_to_g2(ctx.h, bytes(64), 0x80000000 | 64, 1, b"dst", 3, ctypes.create_string_buffer(192)),
                   "lsg_hash_to_g2")


# ---- 8. nothing moved
def test_unmarked_packages_launch_what_they_did_and_reserved_contexts_allocate_nothing(pkg65):
    from lodestar_amd._native import Context, PreparedJobs
    c = Context(0)
    try:
        good = set(pkg65.good())
        shape = [(p, n, f) for p, n, f in pkg65.shape if all(i in good for i in range(p, p + n))]
        n_sets = sum(n for _, n, _ in shape)
        c.reserve(n_sets, max_pks=n_sets, max_msg_bytes=160 * n_sets, n_slots=2)
        root_jobs, obj_jobs = PreparedJobs(pkg65.jobs("root", shape)), PreparedJobs(pkg65.jobs("object", shape))
        got_r, _ = c.verify_jobs(root_jobs, seed=5)  # warm-up, in root form
        names_r = names(c)
        assert norm(got_r) == [(1, 0)] * len(shape) and "k_msg_roots" not in names_r
        before = c.allocation_count()
        for k in range(10):
            assert c.verify_jobs(obj_jobs, seed=6 + k)[0] == got_r
        assert c.allocation_count() == before
        names_o = names(c)
        # the marked package runs one more kernel, directly before k_expand_msg
        at = names_o.index("k_msg_roots")
        assert names_o[at + 1] == "k_expand_msg" and names_o[:at] + names_o[at + 1:] == names_r
    finally:
        c.close()


# ---- 9. Node
def test_node_job_mixing_roots_and_objects(ctx, keys, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: one job mixing signingRoot and
    signingObject sets of every kind and key form; valid, then with one object changed."""
    import json
    import os
    import shutil
    import subprocess
    from oracle.fields import R
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(os.path.join(here, "..", "lodestar_amd", "napi", "lsg_napi.node")), "N-API addon not built"
    sks, pks = keys
    rng = random.Random(55)
    committee = [rng.randrange(64) for _ in range(40)]
    bits = [1 if rng.random() < 0.8 else 0 for _ in committee]
    raw = bytearray(5)
    for j, b in enumerate(bits):
        raw[j >> 3] |= b << (j & 7)
    part = [r for r, b in zip(committee, bits) if b]
    sets, agg, roots, sigs = [], [], [], []
    forms = list(mo.KINDS) + [PLAIN32, 128, 128]
    for i, form in enumerate(forms):
        signers = [i] if i < 8 else ([3, 4, 5] if i == 8 else part)
        key = {"pubkeys": [pks[s].hex() for s in signers]} if i < 8 else (
            {"indices": signers} if i == 8 else {"committee": 7, "bits": bytes(raw).hex(), "bit_len": 40})
        if form == PLAIN32:
            root = rng.randbytes(32)
            msg = {"root": root.hex()}
        else:
            obj, dom = rng.randbytes(form), rng.randbytes(32)
            root = mo.signing_root(obj, dom)
            msg = {"obj": obj.hex(), "domain": dom.hex()}
        sig = ctx.sign([sum(sks[s] for s in signers) % R], [root])[0]
        sets.append(dict(key, sig=sig.hex(), **msg))
        agg.append(g1_serialize(ov.aggregate_pubkeys([ov.public_key_from_bytes(pks[s]) for s in signers])))
        roots.append(root)
        sigs.append(sig)
    assert co.verify_each(agg, roots, sigs) == [1] * len(forms)
    changed = bytearray(bytes.fromhex(sets[4]["obj"]))
    changed[80] ^= 1  # the DepositMessage's amount
    assert co.verify_each([agg[4]], [mo.signing_root(bytes(changed), bytes.fromhex(sets[4]["domain"]))], [sigs[4]]) == [0]
    att = rng.randbytes(128)
    cases = {"pks": [k.hex() for k in pks], "committee_id": 7, "committee": committee, "sets": sets,
             "forged": {"set": 4, "obj": bytes(changed).hex()},
             "roots": {"obj": att.hex(), "domain": sets[0]["domain"], "root": mo.signing_root(att, bytes.fromhex(sets[0]["domain"])).hex()}}
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(here, "js", "test_msg_objects_gpu.js"), str(f)], capture_output=True,
                       text=True, timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "msg objects gpu ok" in r.stdout, r.stdout + r.stderr
