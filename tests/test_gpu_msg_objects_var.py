"""Sets whose message is a variable-size SSZ object + domain on the GPU (a kind tag in the
LSG_MSG_OBJECT length word: AggregateAndProof, phase0 and EIP-7549) and altair's
ContributionAndProof among the fixed kinds: k_msg_roots_var computes a tagged message's signing
root with one 64-lane workgroup, as the package's first stage.  Expected roots come from
tests/msgobjects_var.py (oracle/interop.py's helpers, the bitlist merkleized the naive way;
unpinned beyond the SSZ spec), expected verdicts from tests/cpu_oracle.py's worker.ts rules over
those roots; every object-form package is also compared with the same package in root form
under the same seed.  Every comparison is exact.  Every test here needs an MI355X."""
import ctypes
import hashlib
import random

import pytest

from oracle import verifier as ov
from oracle.curves import g1_serialize
from oracle.fields import R
from oracle.interop import interop_secret_key
from tests import cpu_oracle as co
from tests import msgobjects as mo
from tests import msgobjects_var as mv

pytestmark = pytest.mark.gpu
B = 1  # LSG_JOB_BATCHABLE
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job")
KINDS = (mv.AGG_PROOF, mv.AGG_PROOF_ELECTRA)


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    sks = [interop_secret_key(i) for i in range(64)]
    pks = ctx.sk_to_pk(sks)
    assert ctx.pubkey_table_set(0, pks) == [0] * 64
    return sks, pks


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


# ---- 1. roots
@pytest.mark.parametrize("kind", KINDS)
def test_direct_roots(ctx, kind):
    cs = mv.cases(kind)
    rng = random.Random(kind)
    for n in (1, 2, 63, 64, 65):
        # objects of mixed lengths back to back: successive payloads start at every alignment
        pick = cs if n == 65 else rng.sample(cs, min(n, len(cs)))
        pick = (pick * 3)[:n]
        objs, doms, want = [p[2] for p in pick], [p[3] for p in pick], [p[4] for p in pick]
        assert ctx.object_signing_roots_var(kind, objs, doms) == want, (kind, n)
        assert "k_msg_roots_var" in names(ctx)
        roots = {p[2]: p[5] for p in pick}  # the objects' own roots: the signing root under another domain
        assert ctx.object_signing_roots_var(kind, objs, doms[0]) == [mv.signing_root(roots[o], doms[0]) for o in objs], (kind, n)
    assert len({(sum(len(p[2]) + 32 for p in cs[:k])) % 8 for k in range(len(cs))}) == 8  # every byte alignment
    every = ctx.object_signing_roots_var(kind, [p[2] for p in cs], [p[3] for p in cs])
    assert every == [p[4] for p in cs]  # each of the issue's bit counts, zero, one and random bits
    good = cs[4][2]
    for bad in (good[:8] + b"\x6d" + good[9:], good[:-1] + b"\0", good[:mv.BITS_OFF[kind]]):
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            ctx.object_signing_roots_var(kind, [good, bad], cs[4][3])
    for k in (0, 3, 127):
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            ctx.object_signing_roots_var(k, [good], cs[4][3])
    assert ctx.object_signing_roots_var(kind, [good], cs[4][3]) == [cs[4][4]]  # the context stays usable


def test_direct_roots_contribution_and_proof(ctx):
    rng = random.Random(264)
    for n in (1, 63, 64, 65):
        objs, doms = [rng.randbytes(264) for _ in range(n)], [rng.randbytes(32) for _ in range(n)]
        want = [mv.signing_root(mv.contribution_and_proof_root(o), d) for o, d in zip(objs, doms)]
        assert ctx.object_signing_roots(objs, doms) == want
        assert ctx.object_signing_roots(objs, doms[0]) == [mv.signing_root(mv.contribution_and_proof_root(o), doms[0]) for o in objs]


# ---- 2, 3. packages
class Package:
    """Gossip aggregate jobs [Slot object, tagged AggregateAndProof, AttestationData object with
    keys by index], contribution jobs [SyncAggregatorSelectionData object, ContributionAndProof
    object, Root object with keys by index] and jobs of one plain 32-byte message, in object
    form and in root form.  wrong: job -> "other" (the signature is over another object) or
    "bit" (a participation bit of the signed AggregateAndProof flipped after signing)."""

    def __init__(self, ctx, keys, tag, n_jobs, wrong=None, not_batchable=()):
        from lodestar_amd._native import MsgObject, PkIndices
        sks, pks = keys
        wrong = wrong or {}
        rng = random.Random(hashlib.sha256(tag.encode()).digest())
        self.obj_sets, self.root_sets, self.shape = [], [], []
        agg_pk, msgs, sigs, to_sign, sk_of = [], [], [], [], []
        sizes = {mv.AGG_PROOF: (450, 0, 2048, 257), mv.AGG_PROOF_ELECTRA: (28800, 16385, 131072, 1)}
        for j in range(n_jobs):
            first = len(msgs)
            dom = rng.randbytes(32)
            a = rng.randrange(64)
            part = sorted(rng.sample(range(64), 3))
            form = j % 4
            if form == 3:  # a plain message
                m = rng.randbytes(32)
                sets = [([a], m, m)]
            elif form == 2:  # sync_committee_contribution_and_proof
                sel, cap, blk = rng.randbytes(16), rng.randbytes(264), rng.randbytes(32)
                sets = [([a], MsgObject(sel, dom), mo.signing_root(sel, dom)),
                        ([a], MsgObject(cap, dom), mv.signing_root(mv.contribution_and_proof_root(cap), dom)),
                        (part, MsgObject(blk, dom), mo.signing_root(blk, dom))]
            else:  # beacon_aggregate_and_proof
                kind = KINDS[form]
                n_bits = sizes[kind][(j // 4) % 4]
                slot, data = rng.randbytes(8), rng.randbytes(128)
                obj, root = mv.make_agg_proof(kind, mv.bits_of(n_bits, "random", rng), rng)
                sets = [([a], MsgObject(slot, dom), mo.signing_root(slot, dom)),
                        ([a], MsgObject(obj, dom, kind), mv.signing_root(root, dom)),
                        (part, MsgObject(data, dom), mo.signing_root(data, dom))]
            for k, (signers, m_obj, m_root) in enumerate(sets):
                signed = m_root
                if wrong.get(j) == "other" and k == min(1, len(sets) - 1):
                    signed = hashlib.sha256(m_root).digest()
                if wrong.get(j) == "bit" and k == 1:
                    assert form < 2
                    flipped = bytearray(m_obj.obj)
                    flipped[mv.BITS_OFF[m_obj.kind]] ^= 1  # participation bit 0
                    m_obj = MsgObject(bytes(flipped), m_obj.domain, m_obj.kind)
                    att = self._root_of(bytes(flipped), m_obj.kind)
                    m_root = mv.signing_root(att, dom)
                    assert m_root != signed
                pk = [pks[signers[0]]] if len(signers) == 1 else PkIndices(signers)
                agg_pk.append(pks[signers[0]] if len(signers) == 1 else g1_serialize(
                    ov.aggregate_pubkeys([ov.public_key_from_bytes(pks[s]) for s in signers])))
                sk_of.append(sum(sks[s] for s in signers) % R)
                to_sign.append(signed)
                msgs.append(m_root)
                self.obj_sets.append([pk, m_obj, None])
                self.root_sets.append([pk, m_root, None])
            self.shape.append((first, len(sets), 0 if j in not_batchable else B))
        sigs = ctx.sign(sk_of, to_sign)
        for i, s in enumerate(sigs):
            self.obj_sets[i][2] = self.root_sets[i][2] = s
        self.per_set = co.verify_each(agg_pk, msgs, sigs)
        bad_jobs = sorted(j for j, (p, c, _) in enumerate(self.shape) if any(v != 1 for v in self.per_set[p:p + c]))
        assert bad_jobs == sorted(wrong), (bad_jobs, wrong)
        self.exp, self.retries, self.success = co.expected_jobs(
            [list(range(p, p + c)) for p, c, _ in self.shape], [bool(f & B) for _, _, f in self.shape], self.per_set)
        self.n_tagged = sum(1 for _, m, _ in self.obj_sets if getattr(m, "kind", 0))

    @staticmethod
    def _root_of(obj, kind):
        """hash_tree_root of a serialized AggregateAndProof, by tests/msgobjects_var.py's rules"""
        off = mv.BITS_OFF[kind]
        raw = obj[off:]
        n = 8 * (len(raw) - 1) + raw[-1].bit_length() - 1
        bits = [(raw[k >> 3] >> (k & 7)) & 1 for k in range(n)]
        from oracle import interop as io
        cb = obj[336:344] + bytes(24) if kind == mv.AGG_PROOF_ELECTRA else bytes(32)
        att = io._merkleize([mv.bitlist_root(bits, mv.LIMIT_BITS[kind]), io.attestation_data_root(obj[112:240]),
                             io.htr_bytes_vector(obj[240:336]), cb])
        return io._merkleize([mv.u64(obj[:8]), att, io.htr_bytes_vector(obj[12:108]), bytes(32)])

    def sets(self, form):
        return [tuple(s) for s in (self.obj_sets if form == "object" else self.root_sets)]

    def jobs(self, form, shape=None):
        flat = self.sets(form)
        return [(flat[p:p + c], f) for p, c, f in (shape or self.shape)]

    def good_shape(self):
        return [(p, c, f) for (p, c, f), e in zip(self.shape, self.exp) if e == (1, 0)]


@pytest.fixture(scope="module")
def pkg7(ctx, keys):
    return Package(ctx, keys, "seven", 7, wrong={1: "bit", 4: "other"}, not_batchable=(2,))


@pytest.fixture(scope="module")
def pkg65(ctx, keys):
    p = Package(ctx, keys, "sixty-five", 65, wrong={9: "bit", 16: "other", 30: "other"}, not_batchable=(3, 13, 23, 33, 43))
    assert sum(1 for _, _, f in p.shape if f & B) >= 32 and p.retries >= 1  # chunks, and a fallback
    return p


def check_both_forms(c, pkg, seed):
    got_o, st_o = c.verify_jobs(pkg.jobs("object"), seed=seed)
    assert "k_msg_roots_var" in names(c) and "k_msg_roots" in names(c)
    got_r, st_r = c.verify_jobs(pkg.jobs("root"), seed=seed)
    assert "k_msg_roots_var" not in names(c) and "k_msg_roots" not in names(c)
    assert norm(got_o) == pkg.exp, (norm(got_o), pkg.exp)
    assert got_o == got_r
    assert [st_o[k] for k in COUNTERS] == [st_r[k] for k in COUNTERS]
    assert (st_o["batch_retries"], st_o["batch_sigs_success"], st_o["key_error"]) == (pkg.retries, pkg.success, 0), st_o


def lone(ctx, keys, kind, n_bits, forged, seed):
    from lodestar_amd._native import MsgObject
    sks, pks = keys
    rng = random.Random(seed)
    dom = rng.randbytes(32)
    if kind == 0:
        obj = rng.randbytes(264)
        root = mv.signing_root(mv.contribution_and_proof_root(obj), dom)
    else:
        obj, r = mv.make_agg_proof(kind, mv.bits_of(n_bits, "random", rng), rng)
        root = mv.signing_root(r, dom)
    sig = ctx.sign([sks[5]], [hashlib.sha256(root).digest() if forged else root])[0]
    assert co.verify_each([pks[5]], [root], [sig]) == [0 if forged else 1]
    return ([pks[5]], MsgObject(obj, dom, kind), sig), ([pks[5]], root, sig)


@pytest.mark.parametrize("kind,n_bits", [(0, 0), (mv.AGG_PROOF, 450), (mv.AGG_PROOF_ELECTRA, 28800)])
def test_lone_sets(ctx, keys, kind, n_bits):
    """packages of one set: the lone, unscaled path"""
    for forged in (False, True):
        so, sr = lone(ctx, keys, kind, n_bits, forged, seed=7 * kind + forged)
        want = (0, 0) if forged else (1, 0)
        for flags in (B, 0):
            got_o, st_o = ctx.verify_jobs([([so], flags)], seed=3)
            assert ("k_msg_roots_var" in names(ctx)) == (kind != 0) and ("k_msg_roots" in names(ctx)) == (kind == 0)
            got_r, st_r = ctx.verify_jobs([([sr], flags)], seed=3)
            assert norm(got_o) == norm(got_r) == [want]
            assert [st_o[k] for k in COUNTERS] == [st_r[k] for k in COUNTERS]
        assert ctx.verify_sets([so], seed=5) == ctx.verify_sets([sr], seed=5) == want


@pytest.mark.parametrize("which", ["pkg7", "pkg65"])
def test_packages_of_aggregate_jobs_match_oracle_and_root_form(ctx, which, request):
    pkg = request.getfixturevalue(which)
    check_both_forms(ctx, pkg, seed=3)
    # lsg_batch_partial: byte-equal partials, with the failing sets and without
    good = [i for i, v in enumerate(pkg.per_set) if v == 1]
    for idx in (list(range(len(pkg.per_set))), good):
        so, sr = pkg.sets("object"), pkg.sets("root")
        part_o, errs_o, any_o = ctx.batch_partial([so[i] for i in idx], seed=8)
        assert "k_msg_roots_var" in names(ctx)
        part_r, errs_r, any_r = ctx.batch_partial([sr[i] for i in idx], seed=8)
        assert (part_o, errs_o, any_o) == (part_r, errs_r, any_r)
        assert ctx.final_verify([part_o]) == all(pkg.per_set[i] == 1 for i in idx)
    for idx in (good[:9], good[:9] + [i for i, v in enumerate(pkg.per_set) if v == 0][:1]):
        so, sr = pkg.sets("object"), pkg.sets("root")
        got = ctx.verify_sets([so[i] for i in idx], seed=9)
        assert got == ctx.verify_sets([sr[i] for i in idx], seed=9) == ((1, 0) if len(idx) == 9 else (0, 0))


# ---- 4. dedup
def test_sets_sharing_a_tagged_object_share_its_root(ctx, keys):
    from lodestar_amd._native import MsgObject
    sks, pks = keys
    rng = random.Random(77)
    obj, root = mv.make_agg_proof(mv.AGG_PROOF, mv.bits_of(450, "random", rng), rng)
    obj2, root2 = mv.make_agg_proof(mv.AGG_PROOF_ELECTRA, mv.bits_of(300, "random", rng), rng)
    d0, d1 = rng.randbytes(32), rng.randbytes(32)
    pairs = [(obj, d0, mv.AGG_PROOF), (obj, d1, mv.AGG_PROOF), (obj2, d0, mv.AGG_PROOF_ELECTRA)]
    roots = [mv.signing_root(root, d0), mv.signing_root(root, d1), mv.signing_root(root2, d0)]
    assert len(set(roots)) == 3
    which = [i % 3 for i in range(40)]
    sigs = ctx.sign(sks[:41], [roots[w] for w in which] + [roots[1]])
    sigs[17] = ctx.sign([sks[17]], [roots[(which[17] + 1) % 3]])[0]  # forged: signed over another of the roots
    sets = [([pks[i]], MsgObject(*pairs[which[i]]), sigs[i]) for i in range(40)]
    sets.append(([pks[40]], roots[1], sigs[40]))  # a plain message that equals an object's root
    per_set = co.verify_each(pks[:41], [roots[w] for w in which] + [roots[1]], sigs)
    assert [i for i, v in enumerate(per_set) if v != 1] == [17]
    exp, retries, success = co.expected_jobs([[i] for i in range(41)], [True] * 41, per_set)
    got, stats = ctx.verify_jobs([([s], B) for s in sets], seed=13)
    assert norm(got) == exp and exp.count((0, 0)) == 1
    assert (stats["batch_retries"], stats["batch_sigs_success"]) == (retries, success)
    t = dict(ctx.last_kernel_times())
    assert "k_msg_roots_var" in t and "k_msg_roots" not in t and "k_h2c_gather" in t  # four staged messages for 41 sets
    part, errs, anyerr = ctx.batch_partial([s for i, s in enumerate(sets) if i != 17], seed=2)
    assert not anyerr and ctx.final_verify([part])


# ---- 5. other routes
def fresh(keys, **kw):
    from lodestar_amd._native import Context
    c = Context(**kw) if kw else Context(0)
    assert c.pubkey_table_set(0, keys[1]) == [0] * 64
    return c


def test_coalesced_packages(keys, pkg7):
    c = fresh(keys)
    try:
        c.set_coalesce(4096, 1)  # one launch in flight: the rest wait and go out together
        parts = [pkg7.shape[0:2], pkg7.shape[2:3], pkg7.shape[3:7]]
        tickets = [c.submit_jobs(pkg7.jobs("object", sh), seed=29) for sh in parts]
        assert all(t is not None and t[0] >> 8 & 255 == 4 for t in tickets)  # coalesced tickets
        got = [g for t in tickets for g in c.wait_jobs(t)[0]]
        assert norm(got) == pkg7.exp
        tickets = [c.submit_jobs(pkg7.jobs("root", sh), seed=29) for sh in parts]
        assert got == [g for t in tickets for g in c.wait_jobs(t)[0]]
    finally:
        c.close()


def test_multi_device_duplicate_ids(keys, pkg7):
    c = fresh(keys, devices=[0, 0])
    try:
        assert c.device_count() == 2
        got, stats = c.verify_jobs(pkg7.jobs("object"), seed=31)
        assert norm(got) == pkg7.exp and stats["key_error"] == 0
        assert got == c.verify_jobs(pkg7.jobs("root"), seed=31)[0]
    finally:
        c.close()


def test_node_protocol(ctx, pkg7):
    good = pkg7.jobs("object", pkg7.good_shape())
    t = ctx.submit_jobs(good, seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and ctx.final_verify([part])
    assert norm(ctx.wait_jobs_node(t, 1)[0]) == [(1, 0)] * len(good)
    t = ctx.submit_jobs(pkg7.jobs("object"), seed=37)
    part, has = ctx.jobs_partial(t)
    assert has and not ctx.final_verify([part])
    assert norm(ctx.wait_jobs_node(t, 0)[0]) == pkg7.exp


# ---- 6. message cache
def test_message_cache_bypasses_tagged_messages(keys, pkg7):
    c = fresh(keys)
    try:
        want = c.verify_jobs(pkg7.jobs("object"), seed=41)[0]
        c.msg_cache_set(256)
        before = c.msg_cache_stats()["bypassed"]
        for k in range(2):  # the second package finds the cacheable messages; the tagged ones are hashed again
            assert c.verify_jobs(pkg7.jobs("object"), seed=41)[0] == want
            assert "k_msg_roots_var" in names(c)
        distinct_long = len({(m.tobytes(), m.kind) for _, m, _ in pkg7.obj_sets if hasattr(m, "kind") and len(m) > 192})
        assert c.msg_cache_stats()["bypassed"] - before == 2 * distinct_long and pkg7.n_tagged > 0
    finally:
        c.close()


# ---- 7. arguments
def test_argument_errors_leave_the_context_usable(ctx, keys, pkg7):
    from lodestar_amd._native import LSG_ERR_INVALID_ARG, LsgJob, LsgJobResult, MsgObject, SetBuffer
    rng = random.Random(3)
    good_sets = pkg7.sets("object")
    plain = next(s for s in good_sets if not hasattr(s[1], "kind"))
    bads = []
    for kind in KINDS:
        obj, _ = mv.make_agg_proof(kind, mv.bits_of(300, "random", rng), rng)
        off, dom = mv.BITS_OFF[kind], bytes(32)
        full = mv.make_agg_proof(kind, [1] * mv.LIMIT_BITS[kind], rng)[0]
        bads += [MsgObject(obj[:8] + b"\x6d" + obj[9:], dom, kind),         # the outer offset
                 MsgObject(obj[:108] + b"\0" + obj[109:], dom, kind),       # the inner offset
                 MsgObject(obj[:-1] + b"\0", dom, kind),                    # a zero last byte
                 MsgObject(full[:-1] + b"\x02", dom, kind),                 # one bit over the limit
                 MsgObject(full + b"\x01", dom, kind),                      # a byte too long
                 MsgObject(obj[:off], dom, kind),                           # no bitlist byte
                 MsgObject(obj, dom, 3 - kind),                             # the other kind's layout
                 MsgObject(obj, dom, 3), MsgObject(obj, dom, 127)]          # unknown tags
    for bad_msg in bads:
        b = SetBuffer([plain, (plain[0], bad_msg, plain[2])])
        for flags in (B, 0):
            job = LsgJob(b.arr, 2, flags)
            t, res, out, errs, anyerr = ctypes.c_uint64(), LsgJobResult(), ctypes.create_string_buffer(576), (ctypes.c_int32 * 2)(), ctypes.c_int32()
            assert ctx.lib.lsg_submit_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(t)) == LSG_ERR_INVALID_ARG
            assert ctx.lib.lsg_verify_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(res), None) == LSG_ERR_INVALID_ARG
        assert ctx.lib.lsg_verify_sets(ctx.h, b.arr, 2, 1, ctypes.byref(res)) == LSG_ERR_INVALID_ARG
        assert ctx.lib.lsg_batch_partial(ctx.h, b.arr, 2, 1, out, errs, ctypes.byref(anyerr)) == LSG_ERR_INVALID_ARG
    check_both_forms(ctx, pkg7, seed=43)  # the next good package is verified correctly
    for kind in KINDS:  # a well-formed length word with msg == NULL
        b = SetBuffer([plain, plain])
        b.arr[1].msg, b.arr[1].msg_len = None, 0x80000000 | (kind << 24) | (mv.BITS_OFF[kind] + 33 + 32)
        for flags in (B, 0):
            job = LsgJob(b.arr, 2, flags)
            t, res, out, errs, anyerr = ctypes.c_uint64(), LsgJobResult(), ctypes.create_string_buffer(576), (ctypes.c_int32 * 2)(), ctypes.c_int32()
            assert ctx.lib.lsg_submit_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(t)) == LSG_ERR_INVALID_ARG
            assert ctx.lib.lsg_verify_jobs(ctx.h, ctypes.byref(job), 1, 1, ctypes.byref(res), None) == LSG_ERR_INVALID_ARG
            assert ctx.lib.lsg_verify_sets(ctx.h, b.arr, 2, 1, ctypes.byref(res)) == LSG_ERR_INVALID_ARG
            assert ctx.lib.lsg_batch_partial(ctx.h, b.arr, 2, 1, out, errs, ctypes.byref(anyerr)) == LSG_ERR_INVALID_ARG
    word = 0x80000000 | (1 << 24) | 401
    with pytest.raises(RuntimeError, match=r"\(1\)"):
        ctx._check(ctx.lib.lsg_hash_to_g2(ctx.h, bytes(401), word, 1, b"dst", 3, ctypes.create_string_buffer(192)), "lsg_hash_to_g2")
    check_both_forms(ctx, pkg7, seed=47)


# ---- 8. nothing moved
def test_untagged_packages_launch_what_they_did_and_reserved_contexts_allocate_nothing(keys, pkg65):
    from lodestar_amd._native import PreparedJobs
    c = fresh(keys)
    try:
        shape = pkg65.good_shape()
        n_sets = sum(n for _, n, _ in shape)
        flat = pkg65.sets("object")
        msg_bytes = sum(len(flat[i][1]) for p, n, _ in shape for i in range(p, p + n))
        c.reserve(n_sets, max_pks=3 * n_sets, max_msg_bytes=msg_bytes, n_slots=2)
        root_jobs, obj_jobs = PreparedJobs(pkg65.jobs("root", shape)), PreparedJobs(pkg65.jobs("object", shape))
        got_r, _ = c.verify_jobs(root_jobs, seed=5)  # warm-up, in root form
        names_r = names(c)
        assert norm(got_r) == [(1, 0)] * len(shape) and not [k for k in names_r if k.startswith("k_msg_roots")]
        before = c.allocation_count()
        for k in range(10):
            assert c.verify_jobs(obj_jobs, seed=6 + k)[0] == got_r
        assert c.allocation_count() == before
        names_o = names(c)
        # the tagged package runs k_msg_roots, then k_msg_roots_var, directly before k_expand_msg
        at = names_o.index("k_msg_roots")
        assert names_o[at:at + 3] == ["k_msg_roots", "k_msg_roots_var", "k_expand_msg"]
        assert names_o[:at] + names_o[at + 2:] == names_r
        # fixed kinds only: exactly what they launched before the tagged form existed
        fixed_only = [(sets, f) for sets, f in pkg65.jobs("object", shape) if not any(getattr(m, "kind", 0) for _, m, _ in sets)]
        c.verify_jobs(fixed_only, seed=5)
        assert "k_msg_roots_var" not in names(c) and "k_msg_roots" in names(c)
    finally:
        c.close()


# ---- 9. Node
def test_node_job_mixing_roots_fixed_and_tagged_objects(ctx, keys, tmp_path):
    """BlsGpuVerifier (Node) -> N-API addon -> C ABI on the GPU: one job mixing signingRoot sets,
    fixed-size signingObject sets and AggregateAndProof objects of both kinds; valid, then with a
    participation bit of one signed object flipped; objectSigningRootsVar against the oracle."""
    import json
    import os
    import shutil
    import subprocess
    if shutil.which("node") is None:
        pytest.skip("node not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(os.path.join(here, "..", "lodestar_amd", "napi", "lsg_napi.node")), "N-API addon not built"
    sks, pks = keys
    rng = random.Random(59)
    names_of = {mv.AGG_PROOF: "AggregateAndProof", mv.AGG_PROOF_ELECTRA: "AggregateAndProofElectra"}
    forms = [("root", 0), ("fixed", 8), ("tagged", (mv.AGG_PROOF, 450)), ("fixed", 128), ("tagged", (mv.AGG_PROOF_ELECTRA, 28800)),
             ("fixed", 264), ("tagged", (mv.AGG_PROOF_ELECTRA, 131072)), ("tagged", (mv.AGG_PROOF, 0)), ("fixed", 16)]
    sets, agg, roots, sigs = [], [], [], []
    for i, (form, arg) in enumerate(forms):
        signers = [i] if i % 3 else [i, i + 20, i + 40]
        key = {"pubkeys": [pks[signers[0]].hex()]} if len(signers) == 1 else {"indices": signers}
        dom = rng.randbytes(32)
        if form == "root":
            root = rng.randbytes(32)
            msg = {"root": root.hex()}
        elif form == "fixed":
            obj = rng.randbytes(arg)
            root = mv.signing_root(mv.contribution_and_proof_root(obj), dom) if arg == 264 else mo.signing_root(obj, dom)
            msg = {"obj": obj.hex(), "domain": dom.hex()}
        else:
            kind, n_bits = arg
            obj, r = mv.make_agg_proof(kind, mv.bits_of(n_bits, "random", rng), rng)
            root = mv.signing_root(r, dom)
            msg = {"obj": obj.hex(), "domain": dom.hex(), "kind": names_of[kind]}
        sig = ctx.sign([sum(sks[s] for s in signers) % R], [root])[0]
        sets.append(dict(key, sig=sig.hex(), **msg))
        agg.append(pks[signers[0]] if len(signers) == 1 else g1_serialize(
            ov.aggregate_pubkeys([ov.public_key_from_bytes(pks[s]) for s in signers])))
        roots.append(root)
        sigs.append(sig)
    assert co.verify_each(agg, roots, sigs) == [1] * len(forms)
    flipped = bytearray(bytes.fromhex(sets[4]["obj"]))
    flipped[mv.BITS_OFF[mv.AGG_PROOF_ELECTRA] + 100] ^= 4  # a participation bit of the Electra aggregate
    changed_root = mv.signing_root(Package._root_of(bytes(flipped), mv.AGG_PROOF_ELECTRA), bytes.fromhex(sets[4]["domain"]))
    assert co.verify_each([agg[4]], [changed_root], [sigs[4]]) == [0]
    direct = []
    for kind in KINDS:
        cs = mv.cases(kind)[::5]
        dom = rng.randbytes(32)
        direct.append({"tag": kind, "domain": dom.hex(), "objs": [c[2].hex() for c in cs],
                       "roots": [mv.signing_root(c[5], dom).hex() for c in cs]})
    cases = {"pks": [k.hex() for k in pks], "sets": sets, "forged": {"set": 4, "obj": bytes(flipped).hex()}, "roots": direct,
             "reserve_msg_bytes": sum(len(s.get("obj", "")) // 2 + 32 for s in sets)}
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(here, "js", "test_msg_objects_var_gpu.js"), str(f)], capture_output=True,
                       text=True, timeout=180)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "msg objects var gpu ok" in r.stdout, r.stdout + r.stderr
