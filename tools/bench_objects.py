#!/usr/bin/env python3
"""Block-shaped packages whose messages are SSZ objects (LSG_MSG_OBJECT)
against the present route: 64 blocks per package, each one non-batchable job of 128 committee +
bits sets, one AttestationData per set.  Two forms, alternating in one process after a warm-up:

  object  the sets carry MsgObject(AttestationData bytes, domain): the package computes its
          signing roots on the device (k_msg_roots) and nothing else crosses the host
  roots   one lsg_attestation_signing_roots call per package (H2D, kernel, D2H, the calling thread
          blocked), its roots written into the package's root sets, then the submit

A leg runs for at least --seconds and ends with every package waited on.  One JSON line per leg:
sets/s, p50 package latency (for `roots` from the start of the roots call), median submit_us and
the median host time of the roots call.  Then k_msg_roots' own time from lsg_last_kernel_times
for packages of 128 and of blocks x 128 distinct objects.

  python tools/bench_objects.py [--blocks 64] [--seconds 2] [--rounds 2] [--depth 4]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_KEYS = 1024
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PER_BLOCK = 128


def build(ctx, blocks, validators, members, seed=1):
    """-> (PreparedJobs with MsgObject messages, PreparedJobs with 32-byte root messages, the
    AttestationData bytes back to back, the domain, the expected signing roots) over committees
    0 .. blocks * 128 - 1"""
    import hashlib
    import numpy as np
    from lodestar_amd._native import MsgObject, PkBits, PreparedJobs
    sks = [int.from_bytes(hashlib.sha256(b"bench-objects-sk" + i.to_bytes(4, "little")).digest(), "big") % R_ORDER or 1
           for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    if any(ctx.pubkey_table_set(0, [pks[v % N_KEYS] for v in range(validators)])):
        raise SystemExit("pubkey table load failed")
    n_sets = blocks * PER_BLOCK
    committees = [np.random.default_rng(seed * 1000003 + g).integers(0, validators, members, dtype=np.uint32)
                  for g in range(n_sets)]
    if any(ctx.committees_set(0, [c.tolist() for c in committees])):
        raise SystemExit("committee registration failed")
    domain = hashlib.sha256(b"bench-objects-domain").digest()
    # one AttestationData per set: slot, index, beaconBlockRoot, source, target
    datas = []
    for g in range(n_sets):
        slot, index = 1000 + g // PER_BLOCK, g % PER_BLOCK
        h = [hashlib.sha256(b"bench-objects" + bytes([k]) + g.to_bytes(8, "little")).digest() for k in range(3)]
        datas.append(slot.to_bytes(8, "little") + index.to_bytes(8, "little") + h[0] + (slot // 32 - 1).to_bytes(8, "little") + h[1] +
                     (slot // 32).to_bytes(8, "little") + h[2])
    roots = ctx.attestation_signing_roots(datas, domain)
    rng = np.random.default_rng(seed)
    keys, agg = [], []
    for g, c in enumerate(committees):
        bits = rng.random(members) < 0.99
        bits[0] = True
        keys.append(PkBits(g, np.packbits(bits, bitorder="little").tobytes(), members))
        agg.append(sum(sks[v % N_KEYS] for v in c[bits].tolist()) % R_ORDER)
    sigs = ctx.sign(agg, roots)

    def jobs(msgs):
        return [([(keys[b * PER_BLOCK + i], msgs[b * PER_BLOCK + i], sigs[b * PER_BLOCK + i]) for i in range(PER_BLOCK)], 0)
                for b in range(blocks)]
    return (PreparedJobs(jobs([MsgObject(d, domain) for d in datas])), PreparedJobs(jobs([bytes(32)] * n_sets)),
            b"".join(datas), domain, roots)


def roots_into(ctx, pj, data, domain, n_sets, out):
    """the present route's first step: the package's signing roots by one blocking call, written
    over the root messages of pj; returns the host seconds of the call"""
    t0 = time.perf_counter()
    rc = ctx.lib.lsg_attestation_signing_roots(ctx.h, data, n_sets, domain, 0, out)
    dt = time.perf_counter() - t0
    if rc:
        raise SystemExit(f"lsg_attestation_signing_roots failed ({rc})")
    # pj._msg is PreparedJobs' message arena, the bytes every set's msg pointer points into: the
    # root sets' 32-byte messages lie there back to back in set order, so the roots go in as one copy
    ctypes.memmove(pj._msg.ctypes.data, out, 32 * n_sets)
    return dt


def run_leg(ctx, form, pj, n_sets, seconds, depth, roots_args=None, min_packages=0):
    lat, sub, host, flight, done = [], [], [], [], 0
    t0 = time.perf_counter()
    while True:
        more = time.perf_counter() - t0 < seconds or done + len(flight) < min_packages
        if more and len(flight) < depth:
            ts = time.perf_counter()
            if form == "roots":
                host.append(roots_into(ctx, pj, *roots_args))
            t = ctx.submit_jobs(pj)
            if t is not None:
                flight.append((t, ts))
                continue
        if not flight:
            break
        t, ts = flight.pop(0)
        res, st = ctx.wait_jobs(t, raw=True)
        lat.append(time.perf_counter() - ts)
        sub.append(st["submit_us"])
        if any(res[j].status != 1 for j in range(pj.n_jobs)):
            raise SystemExit("a package did not verify")
        done += 1
    dt = time.perf_counter() - t0
    r = {"form": form, "packages": done, "seconds": round(dt, 3), "sets_per_s": round(done * n_sets / dt, 1),
         "p50_ms": round(1e3 * statistics.median(lat), 3), "submit_us": int(statistics.median(sub))}
    if host:
        r["roots_call_host_us"] = round(1e6 * statistics.median(host), 1)
    return r


def kernel_time(ctx, pj, reps=5):
    """median k_msg_roots milliseconds over `reps` synchronous packages"""
    ms = []
    for _ in range(reps):
        res, _ = ctx.verify_jobs(pj)
        if any(r[0] != 1 for r in res):
            raise SystemExit("a package did not verify")
        t = [v for k, v in ctx.last_kernel_times() if k == "k_msg_roots"]
        if len(t) != 1:
            raise SystemExit("k_msg_roots did not run exactly once")
        ms.append(t[0])
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--validators", type=int, default=1 << 16)
    ap.add_argument("--members", type=int, default=128, help="members per committee")
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rounds", type=int, default=2, help="object / roots alternations")
    ap.add_argument("--depth", type=int, default=4, help="packages in flight")
    args = ap.parse_args()
    from lodestar_amd._native import Context, PreparedJobs
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    t0 = time.perf_counter()
    pj_obj, pj_root, data, domain, roots = build(ctx, args.blocks, args.validators, args.members)
    n_sets = args.blocks * PER_BLOCK
    print(f"inputs built in {time.perf_counter() - t0:.1f} s: {n_sets} sets per package", file=sys.stderr)
    ctx.reserve(n_sets, max_pks=(16 + (args.members + 31) // 32) * n_sets, max_msg_bytes=160 * n_sets, n_slots=args.depth)
    out = ctypes.create_string_buffer(32 * n_sets)
    roots_args = (data, domain, n_sets, out)
    roots_into(ctx, pj_root, *roots_args)
    if out.raw != b"".join(roots):
        raise SystemExit("the roots call disagrees with itself")
    legs = {"object": (pj_obj, None), "roots": (pj_root, roots_args)}
    for form, (pj, ra) in legs.items():  # warm-up
        run_leg(ctx, form, pj, n_sets, 0.0, args.depth, ra, min_packages=3)
    rate = {"object": [], "roots": []}
    p50 = {"object": [], "roots": []}
    for rnd in range(args.rounds):
        for form, (pj, ra) in legs.items():
            r = run_leg(ctx, form, pj, n_sets, args.seconds, args.depth, ra)
            r.update({"round": rnd, "sets_per_package": n_sets, "depth": args.depth})
            rate[form].append(r["sets_per_s"])
            p50[form].append(r["p50_ms"])
            print(json.dumps(r), flush=True)
    for form, (pj, ra) in legs.items():  # one package at a time: the latency of a lone package
        r = run_leg(ctx, form, pj, n_sets, args.seconds / 2, 1, ra)
        r.update({"round": "lone", "sets_per_package": n_sets, "depth": 1})
        print(json.dumps(r), flush=True)
    mo, mr = statistics.mean(rate["object"]), statistics.mean(rate["roots"])
    print(json.dumps({"summary": True, "object_sets_per_s": round(mo, 1), "roots_sets_per_s": round(mr, 1),
                      "object_over_roots": round(mo / mr, 4), "object_p50_ms": p50["object"], "roots_p50_ms": p50["roots"]}), flush=True)
    # k_msg_roots alone: one block's 128 objects, and the whole package's
    small = PreparedJobs(_first_block(pj_obj, data, domain))
    for name, pj, n in (("one block", small, PER_BLOCK), ("package", pj_obj, n_sets)):
        print(json.dumps({"kernel": "k_msg_roots", "objects": n, "what": name, "median_us": round(1e3 * kernel_time(ctx, pj), 2)}),
              flush=True)
    ctx.close()


def _first_block(pj_obj, data, domain):
    """the first block's 128 sets again, as a package of their own"""
    from lodestar_amd._native import MsgObject, PkBits
    sets = []
    for i in range(PER_BLOCK):
        s = pj_obj.sets[i]
        nb = 4 + (s.n_pks + 7) // 8
        raw = ctypes.string_at(s.pks, nb)
        sets.append((PkBits(int.from_bytes(raw[:4], sys.byteorder), raw[4:], s.n_pks), MsgObject(data[128 * i:128 * i + 128], domain),
                     ctypes.string_at(s.sig, s.sig_len)))
    return [(sets, 0)]


if __name__ == "__main__":
    main()
