#!/usr/bin/env python3
"""The message cache (lsg_msg_cache_set) against the same context without it, legs
alternating in one process after a warm-up.  One JSON line per leg.

  gossip    bench.py --workload gossip's package -- one batchable job of 128 single-key sets,
            coalescing 4096, depth 64, each ticket waited on its own thread -- whose messages are
            AttestationData objects (LSG_MSG_OBJECT) drawn from the 64 of a "slot"; a new slot
            every 256 packages.  --slots slots are built; when the sequence wraps, the cache leg
            clears the cache (lsg_msg_cache_clear), so that every slot's first packages miss as
            they would live.  Reported: sets/s, p50 package latency, hit rate, and the hash
            stage's share of the kernel time (lsg_last_kernel_times, sampled per wait).
  lone      one set per call (one non-batchable job), its message warm: unloaded latency.
  firehose  bench.py's default shape -- 32,768 single-key sets per package, every message its
            own, one batchable job each, depth 6 -- where the cache cannot help: sets/s and
            submit_us beside cache off.

  python tools/bench_msg_cache.py [--legs 4] [--seconds 2] [--rows 4096] [--only gossip,lone,firehose]
"""
import argparse
import collections
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_KEYS = 1024
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HASH_STAGE = ("k_msg_roots", "k_expand_msg", "k_h2c_prep", "binv_sswu", "k_h2c_map", "k_slp_h2c", "k_h2c_clear",
              "k_h2c_clear_pair", "binv_hash", "k_h2c_affine", "k_h2c_gather", "k_h2c_cache_merge", "k_h2c_cache_store")
PER_SLOT, PKGS_PER_SLOT, GOSSIP_SETS = 64, 256, 128


def h(tag, *ints):
    return hashlib.sha256(tag + b"".join(i.to_bytes(8, "little") for i in ints)).digest()


def make_keys(ctx):
    sks = [int.from_bytes(h(b"bench-msg-cache-sk", i), "big") % R_ORDER or 1 for i in range(N_KEYS)]
    return sks, ctx.sk_to_pk(sks)


def attestation_data(slot, index):
    return (slot.to_bytes(8, "little") + index.to_bytes(8, "little") + h(b"bbr", slot, index) +
            (slot // 32 - 1).to_bytes(8, "little") + h(b"src", slot) + (slot // 32).to_bytes(8, "little") + h(b"tgt", slot))


def build_gossip(ctx, keys, slots):
    """slots * 256 packages of 128 sets; set j of package p: key (p * 128 + j) mod 1024 over one of
    its slot's 64 AttestationData"""
    import random
    from lodestar_amd._native import MsgObject, PreparedJobs
    sks, pks = keys
    domain = h(b"bench-msg-cache-domain")
    out = []
    for s in range(slots):
        datas = [attestation_data(5000 + s, i) for i in range(PER_SLOT)]
        roots = ctx.attestation_signing_roots(datas, domain)
        objs = [MsgObject(d, domain) for d in datas]
        rng = random.Random(s)
        n = PKGS_PER_SLOT * GOSSIP_SETS
        which = [rng.randrange(PER_SLOT) for _ in range(n)]
        sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], [roots[w] for w in which])
        for p in range(PKGS_PER_SLOT):
            sets = [([pks[i % N_KEYS]], objs[which[i]], sigs[i]) for i in range(p * GOSSIP_SETS, (p + 1) * GOSSIP_SETS)]
            out.append(PreparedJobs([(sets, 1)]))
    return out


def build_firehose(ctx, keys, n_packages, n=32768):
    from lodestar_amd._native import PreparedJobs
    sks, pks = keys
    out = []
    for p in range(n_packages):
        msgs = [h(b"firehose", p, i) for i in range(n)]
        sigs = ctx.sign([sks[i % N_KEYS] for i in range(n)], msgs)
        out.append(PreparedJobs([([([pks[i % N_KEYS]], msgs[i], sigs[i])], 1) for i in range(n)]))
    return out


def run_leg(ctx, pkgs, sets_per_package, seconds, depth, on_wrap=None, sample=64):
    """packages in sequence for at least `seconds`, `depth` in flight, each waited on its own thread"""
    lat, sub, ktimes = [], [], []
    seq = [0]

    def wait(t, t_sub):
        res, st = ctx.wait_jobs(t, raw=True)
        return time.perf_counter() - t_sub, t, res, st

    with ThreadPoolExecutor(max_workers=depth) as ex:
        inflight = collections.deque()

        def submit():
            k = seq[0] % len(pkgs)
            if k == 0 and seq[0] and on_wrap:
                on_wrap()
            t = ctx.submit_jobs(pkgs[k])
            if t is None:
                raise SystemExit("pipeline slots exhausted: lower the depth")
            inflight.append(ex.submit(wait, t, time.perf_counter()))
            seq[0] += 1

        t0 = time.perf_counter()
        while len(inflight) < depth:
            submit()
        done = 0
        while inflight:
            dt, t, res, st = inflight.popleft().result()
            if any(res[j].status != 1 for j in range(t[1])):
                raise SystemExit("a package did not verify")
            lat.append(dt)
            sub.append(st["submit_us"])
            done += 1
            if len(ktimes) < sample:
                ktimes.append(ctx.last_kernel_times())
            if time.perf_counter() - t0 < seconds:
                submit()
        wall = time.perf_counter() - t0
    tot = sum(v for kt in ktimes for _, v in kt if v > 0)
    hs = sum(v for kt in ktimes for k, v in kt if v > 0 and k in HASH_STAGE)
    return {"packages": done, "seconds": round(wall, 3), "sets_per_s": round(done * sets_per_package / wall, 1),
            "p50_ms": round(1e3 * statistics.median(lat), 3), "submit_us": int(statistics.median(sub)),
            "hash_stage_share_of_kernel_time": round(hs / tot, 4) if tot else None}


def cache(ctx, rows, reserve):
    ctx.msg_cache_set(rows)
    if rows:
        ctx.reserve(*reserve[0], **reserve[1])


def with_stats(ctx, rows, leg):
    before = ctx.msg_cache_stats()
    r = leg()
    after = ctx.msg_cache_stats()
    r["cache_rows"] = rows
    if rows:
        d = {k: after[k] - before[k] for k in ("lookups", "hits", "pending", "inserts", "full", "evictions")}
        r["hit_rate"] = round(d["hits"] / d["lookups"], 4) if d["lookups"] else None
        r["cache"] = d
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=4, help="legs a side")
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--only", default="gossip,lone,firehose")
    args = ap.parse_args()
    only = args.only.split(",")
    from lodestar_amd._native import Context, PreparedJobs
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    keys = make_keys(ctx)
    sides = (0, args.rows)
    if "gossip" in only:
        t0 = time.perf_counter()
        pkgs = build_gossip(ctx, keys, args.slots)
        print(f"gossip inputs built in {time.perf_counter() - t0:.1f} s: {len(pkgs)} packages", file=sys.stderr)
        ctx.set_coalesce(4096, 2)
        reserve = ((8192,), {"max_msg_bytes": 160 * 8192})
        ctx.reserve(*reserve[0], **reserve[1])
        for rows in sides:  # warm-up
            cache(ctx, rows, reserve)
            run_leg(ctx, pkgs, GOSSIP_SETS, 0.3, 64)
        for leg in range(args.legs):
            for rows in sides:
                cache(ctx, rows, reserve)
                r = with_stats(ctx, rows, lambda: run_leg(ctx, pkgs, GOSSIP_SETS, args.seconds, 64,
                                                          on_wrap=ctx.msg_cache_clear if rows else None))
                r.update({"workload": "gossip", "leg": leg, "sets_per_package": GOSSIP_SETS, "depth": 64, "coalesce": 4096,
                          "messages_per_slot": PER_SLOT, "packages_per_slot": PKGS_PER_SLOT})
                print(json.dumps(r), flush=True)
        ctx.set_coalesce(0, 2)
        if "lone" in only:
            one = PreparedJobs([([_set_of(pkgs[0], 0)], 0)])
            for leg in range(args.legs):
                for rows in sides:
                    cache(ctx, rows, reserve)
                    run_leg(ctx, [one], 1, 0.0, 1)  # (its message is warm from here on)
                    r = with_stats(ctx, rows, lambda: run_leg(ctx, [one], 1, args.seconds / 4, 1))
                    r.update({"workload": "lone", "leg": leg, "sets_per_package": 1, "depth": 1})
                    print(json.dumps(r), flush=True)
        del pkgs
    if "firehose" in only:
        t0 = time.perf_counter()
        pkgs = build_firehose(ctx, keys, 2)
        print(f"firehose inputs built in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        reserve = ((32768,), {"n_slots": 8})
        ctx.reserve(*reserve[0], **reserve[1])
        for rows in sides:
            cache(ctx, rows, reserve)
            run_leg(ctx, pkgs, 32768, 0.0, 6)
        for leg in range(args.legs):
            for rows in sides:
                cache(ctx, rows, reserve)
                r = with_stats(ctx, rows, lambda: run_leg(ctx, pkgs, 32768, args.seconds, 6))
                r.update({"workload": "firehose", "leg": leg, "sets_per_package": 32768, "depth": 6})
                print(json.dumps(r), flush=True)
    ctx.close()


def _set_of(pj, i):
    """set i of a PreparedJobs as a (pks, msg, sig) tuple again"""
    import ctypes
    from lodestar_amd._native import LSG_MSG_KIND_MASK, LSG_MSG_KIND_SHIFT, LSG_MSG_OBJECT, MsgObject
    s = pj.sets[i]
    marked = bool(s.msg_len & LSG_MSG_OBJECT)  # a marked word: marker, kind tag, payload length
    n = s.msg_len & ~(LSG_MSG_OBJECT | LSG_MSG_KIND_MASK) if marked else s.msg_len
    raw = ctypes.string_at(s.msg, n)
    msg = MsgObject(raw[:n - 32], raw[n - 32:], (s.msg_len & LSG_MSG_KIND_MASK) >> LSG_MSG_KIND_SHIFT) if marked else raw
    return ([ctypes.string_at(s.pks, s.pk_len)], msg, ctypes.string_at(s.sig, s.sig_len))


if __name__ == "__main__":
    main()
