"""The message cache on the GPU (lsg_msg_cache_set): hash_to_G2 points kept across
packages, keyed by the staged message bytes.  Every package here also runs on a context
without the cache under the same nonzero seed -- verdicts, error codes, counters and the 576
exported bytes of lsg_jobs_partial must be equal -- and expected verdicts come from
tests/cpu_oracle.py's worker.ts rules (the C oracle over 32-byte messages and signing roots,
the Python oracle for the few messages of another length).  Cache counters are compared exactly.
Every test here needs an MI355X.

Keys are the 64 interop keys; signatures are made with ctx.sign."""
import hashlib
import random
import threading

import pytest

from oracle import verifier as ov
from oracle.interop import interop_secret_key
from tests import blsdata as bd
from tests import cpu_oracle as co
from tests import msgobjects as mo

pytestmark = pytest.mark.gpu
B = 1  # LSG_JOB_BATCHABLE
SEED = 0x5EED5
COUNTERS = ("batch_retries", "batch_sigs_success", "key_error", "key_error_job", "n_final_exps")
HASH_KERNELS = ("k_msg_roots", "k_expand_msg", "k_h2c_prep", "k_h2c_map", "k_slp_h2c", "k_h2c_clear")
ZERO = dict(lookups=0, hits=0, pending=0, inserts=0, evictions=0, bypassed=0, full=0, entries=0)


@pytest.fixture(scope="module")
def ref():
    """the context without a cache"""
    from lodestar_amd._native import Context
    c = Context(0)  # raises NativeUnavailable loudly if the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ref):
    sks = [interop_secret_key(i) for i in range(64)]
    return sks, ref.sk_to_pk(sks)


@pytest.fixture()
def cached():
    """a fresh context; the test chooses the capacity"""
    from lodestar_amd._native import Context
    c = Context(0)
    yield c
    c.close()


def names(c):
    return [k for k, _ in c.last_kernel_times()]


def norm(got):
    return [(g[0], g[1] if g[0] == 2 else 0) for g in got]


def signed_bytes(m):
    from lodestar_amd._native import MsgObject
    return mo.signing_root(m.obj, m.domain) if isinstance(m, MsgObject) else m


def make_sets(ctx, keys, msgs, which, wrong=(), undecodable=(), signer0=0):
    """set i: key (signer0 + i) % 64 over msgs[which[i]] (bytes or MsgObject) -> (sets, per-set oracle outcomes)"""
    sks, pks = keys
    n = len(which)
    ks = [(signer0 + i) % 64 for i in range(n)]
    real = [signed_bytes(msgs[w]) for w in which]
    signed = [hashlib.sha256(m).digest() if i in wrong else m for i, m in enumerate(real)]
    sigs = [None] * n
    for length in sorted(set(len(m) for m in signed)):  # ctx.sign takes messages of one length
        idx = [i for i in range(n) if len(signed[i]) == length]
        for i, s in zip(idx, ctx.sign([sks[ks[i]] for i in idx], [signed[i] for i in idx])):
            sigs[i] = s
    for i in undecodable:
        sigs[i] = bd.corrupt_flip_x_bit((None, None, sigs[i]))[2]
    per_set = [None] * n
    i32 = [i for i in range(n) if len(real[i]) == 32]
    for i, v in zip(i32, co.verify_each([pks[ks[i]] for i in i32], [real[i] for i in i32], [sigs[i] for i in i32])):
        per_set[i] = v
    for i in range(n):
        if per_set[i] is None:
            per_set[i] = 1 if ov.verify_single(ov.public_key_from_bytes(pks[ks[i]]), real[i],
                                               ov.signature_from_bytes(sigs[i])) else 0
    assert [i for i, v in enumerate(per_set) if v == 0] == sorted(wrong), per_set
    assert [i for i, v in enumerate(per_set) if v < 0] == sorted(undecodable), per_set
    return [([pks[ks[i]]], msgs[which[i]], sigs[i]) for i in range(n)], per_set


def expected(shape, per_set):
    """shape: jobs as (first set, count, flags)"""
    return co.expected_jobs([list(range(p, p + c)) for p, c, _ in shape], [bool(f & B) for _, _, f in shape], per_set)


def jobs_of(sets, shape):
    return [(sets[p:p + c], f) for p, c, f in shape]


def run(c, jobs, seed=SEED):
    """-> (results, the counters, the exported partial and its has_batch)"""
    t = c.submit_jobs(jobs, seed=seed)
    assert t is not None
    part = c.jobs_partial(t)
    got, st = c.wait_jobs(t)
    return got, [st[k] for k in COUNTERS], part


def stats(c, *fields):
    st = c.msg_cache_stats()
    assert st["lookups"] == st["hits"] + st["pending"] + st["inserts"] + st["full"], st
    return tuple(st[k] for k in fields) if fields else st


def singles(n, nb_from=None):
    """one batchable job per set; from nb_from on one non-batchable job of the rest"""
    if nb_from is None:
        return [(i, 1, B) for i in range(n)]
    return [(i, 1, B) for i in range(nb_from)] + [(nb_from, n - nb_from, 0)]


# ---- 1. cold, then warm
def test_cold_then_warm_equals_no_cache(ref, cached, keys):
    from lodestar_amd._native import MsgObject
    rng = random.Random(101)
    att = MsgObject(rng.randbytes(128), rng.randbytes(32))  # an AttestationData + domain
    msgs = [rng.randbytes(32), rng.randbytes(32), rng.randbytes(32), att, rng.randbytes(7), rng.randbytes(200)]
    which = [0, 1, 2, 3] * 5 + [4, 5, 0, 3]  # the 7- and the 200-byte message: one set each
    sets, per_set = make_sets(ref, keys, msgs, which, wrong=[6], undecodable=[13])
    shape = singles(24, nb_from=20)
    exp, retries, success = expected(shape, per_set)
    want = run(ref, jobs_of(sets, shape))
    assert norm(want[0]) == exp and want[1][:2] == [retries, success]
    cached.msg_cache_set(64)
    assert stats(cached) == dict(ZERO, capacity=64)
    cold = run(cached, jobs_of(sets, shape))
    assert stats(cached) == dict(ZERO, lookups=5, inserts=5, bypassed=1, entries=5, capacity=64)
    assert "k_h2c_cache_store" in names(cached) and "k_h2c_cache_merge" not in names(cached)
    warm = run(cached, jobs_of(sets, shape))
    assert stats(cached) == dict(ZERO, lookups=10, hits=5, inserts=5, bypassed=2, entries=5, capacity=64)
    assert "k_h2c_cache_merge" in names(cached) and "k_h2c_cache_store" not in names(cached)
    assert "k_expand_msg" in names(cached)  # the bypassed 200-byte message is still hashed
    assert cold == want and warm == want
    # without the bypassed message a warm package launches no hash stage at all
    keep = [i for i in range(24) if which[i] != 5]
    sub = [sets[i] for i in keep]
    sub_shape = singles(23, nb_from=19)
    want_sub = run(ref, jobs_of(sub, sub_shape))
    assert norm(want_sub[0]) == expected(sub_shape, [per_set[i] for i in keep])[0]
    assert run(cached, jobs_of(sub, sub_shape)) == want_sub
    t = names(cached)
    assert not [k for k in HASH_KERNELS if k in t], t
    assert "k_h2c_cache_merge" in t and "k_h2c_gather" in t
    assert stats(cached, "lookups", "hits", "bypassed") == (15, 10, 2)
    # lsg_verify_sets and a lone set come through the same staging path
    assert cached.verify_sets(sub[:5], seed=SEED) == ref.verify_sets(sub[:5], seed=SEED) == (1, 0)
    assert cached.verify_sets(sub[3:4], seed=SEED) == ref.verify_sets(sub[3:4], seed=SEED) == (1, 0)
    assert not [k for k in HASH_KERNELS if k in names(cached)]
    assert cached.verify_sets(sub[5:8], seed=SEED) == ref.verify_sets(sub[5:8], seed=SEED) == (0, 0)
    cached.msg_cache_clear()
    assert stats(cached, "entries", "hits") == (0, 18)
    assert run(cached, jobs_of(sets, shape)) == want
    assert stats(cached, "entries", "hits") == (5, 18)


# ---- 2. entries cross between the kernel path and the small-package programs
@pytest.fixture(scope="module")
def big(ref, keys):
    """2,049 sets over 2,049 messages (one more than LSG_SLP_ITEMS: the kernel path), three of
    them corrupted, with the cache-less context's answer"""
    rng = random.Random(202)
    msgs = [rng.randbytes(32) for _ in range(2049)]
    sets, per_set = make_sets(ref, keys, msgs, list(range(2049)), wrong=[5, 1999], undecodable=[1024])
    want = run(ref, jobs_of(sets, singles(2049)))
    assert "k_h2c_clear" in names(ref) and "k_slp_h2c" not in names(ref)
    exp, retries, success = expected(singles(2049), per_set)
    assert norm(want[0]) == exp and want[1][:2] == [retries, success]
    return msgs, sets, per_set, want


def test_kernel_path_entries_serve_a_small_package(ref, cached, keys, big):
    msgs, sets, per_set, want = big
    cached.msg_cache_set(4096)
    assert run(cached, jobs_of(sets, singles(2049))) == want
    assert stats(cached, "inserts", "entries", "hits") == (2049, 2049, 0)
    pick = [0, 5, 1024, 2048]  # (a forged set and an undecodable one among them)
    small = [sets[i] for i in pick]
    want_small = run(ref, jobs_of(small, singles(4)))
    assert "k_slp_h2c" in names(ref)
    assert norm(want_small[0]) == expected(singles(4), [per_set[i] for i in pick])[0]
    assert run(cached, jobs_of(small, singles(4))) == want_small
    assert stats(cached, "hits", "inserts") == (4, 2049)
    assert not [k for k in HASH_KERNELS if k in names(cached)]


def test_small_package_entries_serve_the_kernel_path(ref, cached, keys, big):
    msgs, sets, per_set, want = big
    cached.msg_cache_set(4096)
    pick = [7, 1000, 2048]
    small = [sets[i] for i in pick]
    assert run(cached, jobs_of(small, singles(3))) == run(ref, jobs_of(small, singles(3)))
    assert "k_slp_h2c" in names(cached)
    assert stats(cached, "inserts", "entries") == (3, 3)
    # those 3 messages plus 2,046 fresh ones: 2,049 sets, the kernel path without the cache
    assert run(cached, jobs_of(sets, singles(2049))) == want
    assert stats(cached, "hits", "inserts", "entries") == (3, 2049, 2049)
    assert "k_h2c_cache_merge" in names(cached) and "k_h2c_cache_store" in names(cached)


# ---- 3. a plain message and the same bytes as a marked object are two entries
def test_plain_and_marked_bytes_are_two_entries(ref, cached, keys):
    from lodestar_amd._native import MsgObject
    rng = random.Random(303)
    root, domain = rng.randbytes(32), rng.randbytes(32)
    msgs = [root + domain, MsgObject(root, domain)]  # 64 plain bytes; the same 64 bytes as a Root + domain
    sets, per_set = make_sets(ref, keys, msgs, [0, 1, 0, 1])
    assert per_set == [1, 1, 1, 1]
    # signatures swapped between the two forms do not verify: the entries must not be confused
    swapped = [(sets[0][0], msgs[1], sets[0][2]), (sets[1][0], msgs[0], sets[1][2])]
    shape = [(0, 2, 0), (2, 1, B), (3, 1, B)]
    cached.msg_cache_set(16)
    want = run(ref, jobs_of(sets, shape))
    assert norm(want[0]) == [(1, 0)] * 3
    assert run(cached, jobs_of(sets, shape)) == want
    assert stats(cached, "lookups", "inserts", "entries") == (2, 2, 2)
    assert run(cached, jobs_of(sets, shape)) == want
    assert stats(cached, "lookups", "hits", "entries") == (4, 2, 2)
    for s in swapped:
        assert cached.verify_sets([s], seed=SEED) == ref.verify_sets([s], seed=SEED) == (0, 0)
    assert stats(cached, "lookups", "hits", "entries") == (6, 4, 2)


# ---- 4. pending rows, pins and replacement with nothing waited in between
def test_capacity_4_without_waits(ref, cached, keys):
    rng = random.Random(404)
    msgs = [rng.randbytes(32) for _ in range(8)]
    lo, per_lo = make_sets(ref, keys, msgs, [0, 1, 2, 3, 0, 1], wrong=[4])
    hi, per_hi = make_sets(ref, keys, msgs, [4, 5, 6, 7, 6, 7], undecodable=[1], signer0=9)
    shape = singles(6)
    exp_lo, exp_hi = expected(shape, per_lo)[0], expected(shape, per_hi)[0]
    cached.msg_cache_set(4)
    ta = cached.submit_jobs(jobs_of(lo, shape), seed=SEED)
    tb = cached.submit_jobs(jobs_of(hi, shape), seed=SEED)
    # B found every row pending: it hashed its messages itself and stored nothing
    assert stats(cached, "lookups", "hits", "inserts", "full", "pending", "entries") == (8, 0, 4, 4, 0, 0)
    assert norm(cached.wait_jobs(tb)[0]) == exp_hi
    assert norm(cached.wait_jobs(ta)[0]) == exp_lo
    assert stats(cached, "inserts", "entries") == (4, 4)
    assert run(cached, jobs_of(lo, shape)) == run(ref, jobs_of(lo, shape))  # C
    assert stats(cached, "lookups", "hits") == (12, 4)
    assert not [k for k in HASH_KERNELS if k in names(cached)]
    got_d = run(cached, jobs_of(hi, shape))  # D: every row had its second chance, then went
    assert stats(cached, "lookups", "inserts", "evictions", "entries") == (16, 8, 4, 4)
    got_e = run(cached, jobs_of(lo, shape))  # E
    assert stats(cached, "lookups", "hits", "inserts", "evictions", "full", "pending") == (20, 4, 12, 8, 4, 0)
    assert norm(got_d[0]) == exp_hi and norm(got_e[0]) == exp_lo
    assert got_d == run(ref, jobs_of(hi, shape)) and got_e == run(ref, jobs_of(lo, shape))
    # a package whose message is in flight in another slot hashes it itself (pending)
    fresh = [rng.randbytes(32)]
    one, _ = make_sets(ref, keys, fresh, [0, 0])
    t1 = cached.submit_jobs(jobs_of(one, singles(2)), seed=SEED)
    t2 = cached.submit_jobs(jobs_of(one, singles(2)), seed=SEED)
    assert stats(cached, "lookups", "pending", "inserts") == (22, 1, 13)
    assert cached.wait_jobs(t2)[0] == cached.wait_jobs(t1)[0] == [(1, 0)] * 2


# ---- 5. coalesced launches
def test_coalesced_packages_with_the_cache(ref, cached, keys):
    rng = random.Random(505)
    msgs = [rng.randbytes(32) for _ in range(4)]
    pkgs, exps = [], []
    for k in range(8):
        sets, per_set = make_sets(ref, keys, msgs, [i % 4 for i in range(16)], wrong=[k] if k % 2 else (),
                                  undecodable=() if k % 2 else [15 - k], signer0=5 * k)
        pkgs.append(jobs_of(sets, singles(16)))
        exps.append(expected(singles(16), per_set))
    cached.msg_cache_set(64)
    cached.set_coalesce(128, 2)
    tickets = [cached.submit_jobs(p, seed=SEED) for p in pkgs]
    assert all(t is not None for t in tickets)
    got = {i: cached.wait_jobs(tickets[i]) for i in (3, 0, 7, 5, 1, 6, 2, 4)}  # waits in any order
    for i, p in enumerate(pkgs):
        want, wst = ref.verify_jobs(p, seed=SEED)
        res, st = got[i]
        assert res == want and norm(res) == exps[i][0], (i, res, want)
        for k in COUNTERS[:4]:
            assert st[k] == wst[k], (i, k)
        assert (st["batch_retries"], st["batch_sigs_success"]) == exps[i][1:]
    st = stats(cached)
    assert st["bypassed"] == 0 and st["inserts"] == 4 == st["entries"] and st["hits"] + st["pending"] > 0
    # once more: every launch finds its four messages
    tickets = [cached.submit_jobs(p, seed=SEED) for p in pkgs]
    for i in range(8):
        assert cached.wait_jobs(tickets[i])[0] == got[i][0]
    after = stats(cached)
    assert after["hits"] - st["hits"] == after["lookups"] - st["lookups"] > 0 and after["inserts"] == 4


# ---- 6. a context over two devices: one cache each
def test_two_devices_each_keep_a_cache(ref, keys):
    from lodestar_amd._native import Context
    rng = random.Random(606)
    msgs = [rng.randbytes(32) for _ in range(5)]
    sets, per_set = make_sets(ref, keys, msgs, [i % 5 for i in range(20)], wrong=[3], undecodable=[17])
    shape = singles(20, nb_from=18)
    want, wst = ref.verify_jobs(jobs_of(sets, shape), seed=SEED)
    assert norm(want) == expected(shape, per_set)[0]
    c, ref2 = Context(devices=[0, 0]), Context(devices=[0, 0])
    try:
        # (each device counts the retries of its own share: the counters are those of a
        # cache-less context over the same two devices)
        want2, wst = ref2.verify_jobs(jobs_of(sets, shape), seed=SEED)
        assert want2 == want
        c.msg_cache_set(32)
        assert stats(c, "capacity") == (64,)
        for rnd in range(2):
            got, st = c.verify_jobs(jobs_of(sets, shape), seed=SEED)
            assert got == want
            assert [st[k] for k in COUNTERS[:4]] == [wst[k] for k in COUNTERS[:4]]
            # each device staged half the sets: all five messages on both
            assert stats(c, "lookups", "hits", "inserts", "entries") == (10 * (rnd + 1), 10 * rnd, 10, 10)
    finally:
        c.close()
        ref2.close()


# ---- 7. four submitting threads, more messages than rows
def test_four_threads_evict_and_agree_with_the_oracle(ref, cached, keys):
    rng = random.Random(707)
    msgs = [rng.randbytes(32) for _ in range(24)]
    which = [m for m in range(24) for _ in range(6)]
    pool, per_set = make_sets(ref, keys, msgs, which, wrong=[4, 77, 130], undecodable=[50])
    pkgs = []
    for _ in range(40):
        idx = [rng.randrange(len(pool)) for _ in range(32)]
        pkgs.append((jobs_of([pool[i] for i in idx], singles(32)), expected(singles(32), [per_set[i] for i in idx])))
    cached.msg_cache_set(8)
    failures = []

    def worker(mine):
        try:
            for jobs, (exp, retries, success) in mine:
                got, st = cached.verify_jobs(jobs, seed=SEED)
                if norm(got) != exp or (st["batch_retries"], st["batch_sigs_success"]) != (retries, success):
                    failures.append((norm(got), exp))
        except Exception as e:  # noqa: BLE001
            failures.append(repr(e))

    threads = [threading.Thread(target=worker, args=(pkgs[k::4],)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures[:2]
    st = stats(cached)
    assert st["evictions"] > 0 and st["hits"] > 0 and st["entries"] <= 8 and st["bypassed"] == 0


# ---- 8. allocation-free after lsg_reserve; off again
def test_reserved_packages_allocate_nothing_and_off_is_off(ref, cached, keys):
    rng = random.Random(808)
    msgs = [rng.randbytes(32) for _ in range(30)]
    pkgs = []
    for k in range(10):  # each package: 40 sets over 8 messages, 5 of them seen before
        mine = [(3 * k + j) % 30 for j in range(8)]
        sets, per_set = make_sets(ref, keys, msgs, [mine[i % 8] for i in range(40)], wrong=[k], signer0=k)
        pkgs.append((jobs_of(sets, singles(40)), expected(singles(40), per_set)[0]))
    cached.msg_cache_set(16)
    cached.reserve(256, n_slots=2)
    before = cached.allocation_count()
    for jobs, exp in pkgs:
        assert norm(cached.verify_jobs(jobs, seed=SEED)[0]) == exp
    assert cached.allocation_count() == before
    st = stats(cached)
    assert st["hits"] > 0 and st["evictions"] > 0 and st["capacity"] == 16
    cached.msg_cache_set(0)
    assert stats(cached) == dict(ZERO, capacity=0)
    for jobs, exp in pkgs[:2]:
        assert run(cached, jobs) == run(ref, jobs)
        assert "k_h2c_cache_merge" not in names(cached) and "k_h2c_cache_store" not in names(cached)
    assert stats(cached) == dict(ZERO, capacity=0)
