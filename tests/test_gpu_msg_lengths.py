"""hash_to_G2 on the GPU over message and DST lengths (tests/msglens.py): k_expand_msg's own
SHA-256 (lsg_k_hash.hip ShaLds: shal_final's extra block, the 0x80 byte or the alignment padding
completing a block, an empty last block; shal_bytes's 16-byte chunks) and the host side of
messages that differ only in length (lsg_stage.hpp's back-to-back staging and MsgTable,
lsg_msg_cache.hpp).  Before this file every message that reached the device was 32 bytes under
the 43-byte POP DST: b_0 ended 15 bytes into a block, every b_i 13.

Everything is exact: 192 output bytes against the oracle (the Python oracle at the named tails
and the cross pairs, the C oracle elsewhere; tests/test_msg_lengths_host.py pins the two against
each other, hashlib and the host build of the kernel headers at these same cases), verdicts and
counters against oracle/verifier.py's worker.ts rules, exported partials byte for byte.
Signatures of the packages come from oracle.verifier.sign, never from the device.
Every test here needs an MI355X."""
import ctypes
import functools
import random

import pytest

from oracle import hash_to_curve as h2c
from oracle import verifier as ov
from oracle.curves import g2_compress, g2_serialize
from oracle.fields import f12_coeffs
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import msglens as ml
from tests import msgobjects as mo
from tests import msgobjects_var as mv
from tests.test_gpu_parity import _splitmix_rands, oracle_job_results

pytestmark = pytest.mark.gpu
B = 1  # LSG_JOB_BATCHABLE
SEED = 0x5EED9
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job", "n_final_exps")
HASH_KERNELS = ("k_msg_roots", "k_expand_msg", "k_h2c_prep", "k_h2c_map", "k_slp_h2c", "k_h2c_clear")
SUBSET = (0, 9, 17, 33, 56, 64, 129)  # the small package's lengths
APPEND, CUT, LAST = 9, 17, 64  # the lengths whose set gets m || 0x00, m[:-1], m with its last byte changed


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture()
def fresh():
    from lodestar_amd._native import Context
    c = Context(0)
    yield c
    c.close()


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


NAMED_CASES = frozenset(ml.named_cases())


@functools.lru_cache(maxsize=None)
def expected(m, dst=ml.DST_POP):
    """hash_to_G2(m) under dst, computed once per run"""
    if (m, dst) in NAMED_CASES:
        return g2_serialize(h2c.hash_to_g2(m, dst))
    return co.hash_to_g2(m, dst)


# ---- a. the message sweep
@pytest.mark.parametrize("run", ml.chunks(ml.MSG_LENS, 4), ids=ml.chunk_id)
def test_message_sweep(ctx, run):
    """one lsg_hash_to_g2 call per length with its three contents; a failure lists (L, b_0's tail,
    content) of every wrong point"""
    wrong = []
    for L in run:
        msgs = ml.contents(L)
        got = ctx.hash_to_g2(msgs)
        assert "k_expand_msg" in names(ctx)
        assert len(got) == len(msgs)
        for which, (m, g) in enumerate(zip(msgs, got)):
            if g != expected(m):
                wrong.append((L, ml.tail_name(ml.b0_tail(L)), ("zero", "ff", "random")[which] if L else "empty"))
    assert not wrong, wrong


# ---- b. the DST sweep
@pytest.mark.parametrize("run", ml.chunks(ml.DST_LENS, 4), ids=ml.chunk_id)
def test_dst_sweep(ctx, run):
    m = ml.m32()
    wrong = []
    for D in run:
        dst = ml.dst_of(D)
        got, = ctx.hash_to_g2([m], dst=dst)
        if got != expected(m, dst):
            wrong.append((D, ml.tail_name(ml.b0_tail(32, D)), ml.tail_name(ml.bi_tail(D))))
    assert not wrong, wrong


def test_cross_pairs(ctx):
    wrong = []
    for L, D in ml.CROSS:
        m, dst = ml.cross_msg(L), ml.dst_of(D)
        got, = ctx.hash_to_g2([m], dst=dst)
        if got != expected(m, dst):
            wrong.append((L, D, ml.tail_name(ml.b0_tail(L, D)), ml.tail_name(ml.bi_tail(D))))
    assert not wrong, wrong


def test_dst_of_256_bytes_is_refused_and_the_pop_dst_is_restored(ctx):
    from lodestar_amd._native import LSG_ERR_INVALID_ARG
    m = ml.m32()
    out = ctypes.create_string_buffer(192)
    assert ctx.lib.lsg_hash_to_g2(ctx.h, m, 32, 1, bytes(256), 256, out) == LSG_ERR_INVALID_ARG
    assert out.raw == bytes(192)
    with pytest.raises(RuntimeError, match=r"\(%d\)" % LSG_ERR_INVALID_ARG):
        ctx.hash_to_g2([m], dst=bytes(256))
    # the context is usable: the longest DST, then the utility slot's POP DST is back for lsg_sign
    dst = ml.dst_of(255)
    assert ctx.hash_to_g2([m], dst=dst) == [expected(m, dst)]
    assert ctx.hash_to_g2([m], dst=b"") == [expected(m, b"")]
    for msg in (m, ml.rnd_msg(9)):
        sk = bd.sk(3)
        assert ctx.sign([sk], [msg]) == [g2_compress(ov.sign(sk, msg))]
    assert ctx.hash_to_g2([m]) == [expected(m)]


# ---- c, d. one launch, many lengths
def repoint(sets, lens):
    """the package with three sets re-pointed, each keeping its signature: m || 0x00, m[:-1], m
    with its last byte changed -> (sets, the three positions)"""
    out = list(sets)
    at = [lens.index(L) for L in (APPEND, CUT, LAST)]
    for i, f in zip(at, (lambda m: m + b"\x00", lambda m: m[:-1], lambda m: m[:-1] + bytes([m[-1] ^ 0x80]))):
        pks, m, sig = out[i]
        out[i] = (pks, f(m), sig)
    return out, at


def singles(sets):
    return [([s], B) for s in sets]


def oracle_each(sets):
    return [1 if ov.verify_single(ov.public_key_from_bytes(p[0]), m, ov.signature_from_bytes(s)) else 0
            for p, m, s in sets]


class Package:
    """One set per length, each its own batchable job, in a shuffled order: neighbouring lanes of
    k_expand_msg's wave are in different SHA blocks and at different tails.  Keys are interop
    keys, signatures the oracle's.  valid: the oracle's worker.ts answer; bad: three sets
    re-pointed, expectations from the oracle's per-set verdicts (the untouched sets are the
    ones the oracle has just accepted)."""

    def __init__(self, lens, tag):
        self.lens = list(lens)
        random.Random(len(self.lens)).shuffle(self.lens)
        self.sets = []
        for i, L in enumerate(self.lens):
            m = ml.rnd_msg(L, salt=3)
            self.sets.append(([bd.pk_bytes(i % 64)], m, g2_compress(ov.sign(bd.sk(i % 64), m))))
        exp, out = oracle_job_results(singles(self.sets))
        assert exp == [(1, None)] * len(self.sets), tag
        self.valid = ([(1, 0)] * len(self.sets), out["batch_retries"], out["batch_sigs_success"])
        self.bad_sets, self.bad_at = repoint(self.sets, self.lens)
        per_set = [1] * len(self.sets)
        for i, v in zip(self.bad_at, oracle_each([self.bad_sets[i] for i in self.bad_at])):
            per_set[i] = v
        assert [i for i, v in enumerate(per_set) if v != 1] == sorted(self.bad_at)
        n = len(self.sets)
        self.bad = co.expected_jobs([[i] for i in range(n)], [True] * n, per_set)


@pytest.fixture(scope="module")
def pkg131():
    p = Package(range(131), "131")
    assert sorted(p.lens) == list(range(131)) and p.lens != sorted(p.lens)
    return p


@pytest.fixture(scope="module")
def pkg7():
    return Package(SUBSET, "7")


def check_package(c, pkg, hash_kernel):
    other = {"k_h2c_clear": "k_slp_h2c", "k_slp_h2c": "k_h2c_clear"}[hash_kernel]
    for sets, (exp, retries, success) in ((pkg.sets, pkg.valid), (pkg.bad_sets, pkg.bad)):
        got, st = c.verify_jobs(singles(sets), seed=SEED)
        t = names(c)
        assert "k_expand_msg" in t and hash_kernel in t and other not in t, t
        assert norm(got) == exp, [(i, pkg.lens[i], g) for i, (g, e) in enumerate(zip(norm(got), exp)) if g != e]
        assert (st["batch_retries"], st["batch_sigs_success"]) == (retries, success), st
    assert [i for i, e in enumerate(pkg.bad[0]) if e != (1, 0)] == sorted(pkg.bad_at)  # exactly those three
    assert pkg.bad[0].count((0, 0)) == 3 and pkg.bad[1] >= 1


def test_package_of_every_length_small_package_programs(ctx, pkg131):
    """131 sets are below the shipped library's LSG_SLP_ITEMS (2,048): clearing and affine
    conversion run as the small-package program"""
    check_package(ctx, pkg131, "k_slp_h2c")


def test_package_of_every_length_kernel_path(ab_ctx, pkg131, monkeypatch):
    """the same package through k_h2c_clear / k_h2c_affine: the shipped library takes them from
    2,049 sets on, the A/B build with LSG_SLP_ITEMS=0 at any size"""
    monkeypatch.setenv("LSG_SLP_ITEMS", "0")
    check_package(ab_ctx, pkg131, "k_h2c_clear")


def test_package_of_seven_lengths(ctx, pkg7):
    assert sorted(pkg7.lens) == list(SUBSET)
    check_package(ctx, pkg7, "k_slp_h2c")


@pytest.mark.parametrize("which", ["pkg7", "pkg131"])
def test_package_partial_bit_exact_vs_oracle(ctx, which, request):
    """lsg_jobs_partial of the valid package equals the oracle's Miller product under the seeded
    randomizers (as test_shipped_jobs_partial_bit_exact_vs_oracle, over messages of every length)"""
    pkg = request.getfixturevalue(which)
    n = len(pkg.sets)
    t = ctx.submit_jobs(singles(pkg.sets), seed=SEED)
    part, has = ctx.jobs_partial(t)
    assert has
    exp, errs = ov.batch_partial([(p[0], m, s) for p, m, s in pkg.sets], _splitmix_rands(SEED, n))
    assert errs == [0] * n
    assert part == b"".join(int(c[0]).to_bytes(48, "big") + int(c[1]).to_bytes(48, "big") for c in f12_coeffs(exp))
    assert ctx.wait_jobs_node(t, 1)[0] == [(1, 0)] * n


# ---- e. the dedup table over messages that are prefixes of one another
def test_committee_package_over_prefix_siblings(ctx):
    m = ml.rnd_msg(33, salt=5)
    msgs = [m, m + b"\x00", m + b"\x00\x00", m[:-1], b""]
    which = [i % 4 for i in range(40)]
    which[22] = 4  # the empty message once
    sets = []
    for i, w in enumerate(which):
        sets.append(([bd.pk_bytes(i)], msgs[w], g2_compress(ov.sign(bd.sk(i), msgs[w]))))
    exp, out = oracle_job_results(singles(sets))
    assert exp == [(1, None)] * 40
    got, st = ctx.verify_jobs(singles(sets), seed=SEED)
    assert "k_h2c_gather" in names(ctx)  # the messages repeat: staged through MsgTable, hashed once each
    assert got == [(1, 0)] * 40
    assert (st["batch_retries"], st["batch_sigs_success"]) == (out["batch_retries"], out["batch_sigs_success"]) == (0, 40)
    for at, sibling in ((4, 1), (9, 3), (6, 1), (22, 0), (3, 4)):  # m -> m||0, m||0 -> m[:-1], m||00 -> m||0, "" -> m, m[:-1] -> ""
        assert msgs[which[at]] != msgs[sibling]
        bad = list(sets)
        bad[at] = (sets[at][0], msgs[sibling], sets[at][2])
        per_set = [1] * 40
        per_set[at], = oracle_each([bad[at]])
        assert per_set[at] == 0
        exp, retries, success = co.expected_jobs([[i] for i in range(40)], [True] * 40, per_set)
        got, st = ctx.verify_jobs(singles(bad), seed=SEED)
        assert "k_h2c_gather" in names(ctx)
        assert norm(got) == exp and [i for i, g in enumerate(got) if g != (1, 0)] == [at], (at, got)
        assert (st["batch_retries"], st["batch_sigs_success"]) == (retries, success)


# ---- f. object payloads at unaligned offsets of the staged message bytes
def test_objects_staged_after_odd_length_messages(ctx):
    from lodestar_amd._native import MsgObject
    rng = random.Random(606)
    att, dom_a = rng.randbytes(128), rng.randbytes(32)
    agg, agg_root = mv.make_agg_proof(mv.AGG_PROOF, mv.bits_of(450, "random", rng), rng)
    dom_g = rng.randbytes(32)
    forms = [  # (object form, root form): staged at offsets 0, 33, 193, 194 and after the tagged object
        (ml.rnd_msg(33, salt=6),) * 2,
        (MsgObject(att, dom_a), mo.signing_root(att, dom_a)),
        (ml.rnd_msg(1, salt=6),) * 2,
        (MsgObject(agg, dom_g, mv.AGG_PROOF), mv.signing_root(agg_root, dom_g)),
        (ml.rnd_msg(32, salt=6),) * 2,
    ]
    assert len(forms[1][0]) == 160 and (194 + len(forms[3][0])) % 4 != 0  # (the 32-byte root is unaligned too)
    sigs = [g2_compress(ov.sign(bd.sk(i), root)) for i, (_, root) in enumerate(forms)]
    obj_sets = [([bd.pk_bytes(i)], o, sigs[i]) for i, (o, _) in enumerate(forms)]
    root_sets = [([bd.pk_bytes(i)], r, sigs[i]) for i, (_, r) in enumerate(forms)]
    flipped = bytearray(att)
    flipped[127] ^= 1
    forged = (MsgObject(bytes(flipped), dom_a), mo.signing_root(bytes(flipped), dom_a))
    for bad in (False, True):
        o_sets, r_sets = list(obj_sets), list(root_sets)
        if bad:  # the AttestationData changed after signing
            o_sets[1] = (obj_sets[1][0], forged[0], sigs[1])
            r_sets[1] = (root_sets[1][0], forged[1], sigs[1])
        exp, out = oracle_job_results(singles(r_sets))
        assert [e[0] for e in exp] == ([1, 0, 1, 1, 1] if bad else [1] * 5)
        res = {}
        for form, sets in (("object", o_sets), ("root", r_sets)):
            t = ctx.submit_jobs(singles(sets), seed=SEED)
            part = ctx.jobs_partial(t)
            got, st = ctx.wait_jobs(t)
            res[form] = (got, [st[k] for k in COUNTERS], part)
            assert ("k_msg_roots" in names(ctx)) == ("k_msg_roots_var" in names(ctx)) == (form == "object")
            assert [g[0] for g in got] == [e[0] for e in exp] and all(g[1] == 0 for g in got), (form, got)
            assert (st["batch_retries"], st["batch_sigs_success"]) == (out["batch_retries"], out["batch_sigs_success"])
        assert res["object"] == res["root"]


# ---- g. the message cache: its length limit, and entries that are prefixes of one another
def test_message_cache_over_lengths(ctx, fresh):
    m32, m192 = ml.rnd_msg(32, salt=7), ml.rnd_msg(192, salt=7)
    msgs = [ml.rnd_msg(1, salt=7), m32[:-1], m32, m32 + b"\x00", m192[:-1], m192, m192 + b"\x00", b""]
    assert [len(m) for m in msgs] == [1, 31, 32, 33, 191, 192, 193, 0]
    cacheable = [m for m in msgs if 0 < len(m) <= 192]
    sets = []
    for i in range(16):  # two sets per message
        m = msgs[i % 8]
        sets.append(([bd.pk_bytes(i)], m, g2_compress(ov.sign(bd.sk(i), m))))
    sets.append(([bd.pk_bytes(2)], msgs[3], sets[2][2]))   # m || 0x00 under the signature over m
    sets.append(([bd.pk_bytes(13)], msgs[4], sets[13][2]))  # m[:-1] under the signature over m
    per_set = oracle_each(sets)
    assert per_set == [1] * 16 + [0, 0]
    n = len(sets)
    exp, retries, success = co.expected_jobs([[i] for i in range(n)], [True] * n, per_set)

    def run(c, ss):
        t = c.submit_jobs(singles(ss), seed=SEED)
        part = c.jobs_partial(t)
        got, st = c.wait_jobs(t)
        return got, [st[k] for k in COUNTERS], part

    def stats(c, *fields):
        st = c.msg_cache_stats()
        assert st["lookups"] == st["hits"] + st["pending"] + st["inserts"] + st["full"], st
        return tuple(st[k] for k in fields)

    want = run(ctx, sets)
    assert norm(want[0]) == exp and want[1][:2] == [retries, success]
    fresh.msg_cache_set(64)
    cold = run(fresh, sets)
    # one insert per distinct cacheable message: the prefix siblings are entries of their own
    assert stats(fresh, "lookups", "hits", "inserts", "entries", "bypassed") == (6, 0, 6, 6, 2)
    assert "k_h2c_cache_store" in names(fresh) and "k_h2c_cache_merge" not in names(fresh)
    warm = run(fresh, sets)
    assert stats(fresh, "lookups", "hits", "inserts", "entries", "bypassed") == (12, 6, 6, 6, 4)
    assert "k_h2c_cache_merge" in names(fresh) and "k_h2c_cache_store" not in names(fresh)
    assert "k_expand_msg" in names(fresh)  # the 193-byte and the empty message are still hashed
    assert cold == want and warm == want
    # without the two bypassed messages a warm package launches no hash stage at all
    keep = [i for i in range(n) if sets[i][1] in cacheable]
    sub = [sets[i] for i in keep]
    assert len(sub) == 14
    want_sub = run(ctx, sub)
    assert norm(want_sub[0]) == co.expected_jobs([[i] for i in range(14)], [True] * 14, [per_set[i] for i in keep])[0]
    assert run(fresh, sub) == want_sub
    t = names(fresh)
    assert not [k for k in HASH_KERNELS if k in t], t
    assert "k_h2c_cache_merge" in t
    assert stats(fresh, "lookups", "hits", "inserts", "bypassed") == (18, 12, 6, 4)


# ---- h. coalesced launches: message offsets rebased when packages merge
def test_coalesced_mixed_length_packages(ctx, fresh, pkg131):
    at = {L: i for i, L in enumerate(pkg131.lens)}
    pick = lambda sets, lens: singles([sets[at[L]] for L in lens])  # noqa: E731
    pkgs = [
        singles(pkg131.sets[:100]),                         # above the limit: launches on its own, at once
        pick(pkg131.bad_sets, (33, APPEND, 0, 1, 130)),     # held while it runs; one re-pointed set
        pick(pkg131.sets, (56, 3, 129, 64)),
        pick(pkg131.bad_sets, (7, CUT, LAST, 2)),           # two re-pointed sets
    ]
    fresh.set_coalesce(16, 1)
    tickets = [fresh.submit_jobs(p, seed=SEED) for p in pkgs]
    assert all(t is not None for t in tickets)
    assert [t[0] >> 8 & 255 for t in tickets] == [1, 4, 4, 4]  # SLOT_JOBS, then SLOT_MERGE tickets
    got = {i: fresh.wait_jobs(tickets[i]) for i in (2, 0, 3, 1)}
    for i, p in enumerate(pkgs):
        want, wst = ctx.verify_jobs(p, seed=SEED)
        res, st = got[i]
        assert res == want, (i, res, want)
        for k in COUNTERS[:4]:
            assert st[k] == wst[k], (i, k)
    assert [[g[0] for g in got[i][0]] for i in (1, 2, 3)] == [[1, 0, 1, 1, 1], [1] * 4, [1, 0, 0, 1]]
