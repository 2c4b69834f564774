#!/usr/bin/env python3
"""Packages of gossip aggregate jobs whose messages are SSZ objects, the tagged AggregateAndProof
among them (LSG_MSG_OBJECT with a kind tag), against the same packages in root
form.  A job is what validateGossipAggregateAndProof verifies: [selection proof over the Slot,
aggregate-and-proof signature over the AggregateAndProof, aggregate over the AttestationData
with its signers by index], batchable.  Two forms, alternating in one process after a warm-up:

  object  the three sets carry MsgObject(bytes, domain[, kind]): the package computes the signing
          roots on the device (k_msg_roots, k_msg_roots_var)
  roots   the three sets carry 32-byte roots computed before the timed region, so this form
          pays nothing for them: an upper bound for the object form

A leg runs for at least --seconds and ends with every package waited on.  One JSON line per leg
(sets/s, p50 package latency, median submit_us), then a summary with both forms' leg-to-leg
spread.  Then k_msg_roots_var alone, from lsg_last_kernel_times, median of five synchronous
packages of 128 and of 8,192 single-set jobs of each shape (phase0 at 450 bits, Electra at 28,800
and at 131,072 bits), beside k_msg_roots over as many AttestationData objects.

  python tools/bench_objects_var.py [--jobs 256] [--seconds 2] [--rounds 2] [--depth 4] [--no-kernel]
"""
import argparse
import hashlib
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
SHAPES = ((1, 450), (2, 28800), (2, 131072))  # (kind tag, aggregation bits)


def stream(tag, n):
    """n deterministic bytes"""
    out, k = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(tag + k.to_bytes(8, "little")).digest()
        k += 1
    return bytes(out[:n])


_bases = {}


def agg_proof(kind, n_bits, index, salt):
    """a serialized AggregateAndProof (kind 1: phase0, 2: EIP-7549) with n_bits aggregation bits:
    one body per salt, the aggregatorIndex set per object"""
    if (kind, n_bits, salt) not in _bases:
        _bases[(kind, n_bits, salt)] = _agg_proof(kind, n_bits, 0, salt)
    return index.to_bytes(8, "little") + _bases[(kind, n_bits, salt)][8:]


def _agg_proof(kind, n_bits, index, salt):
    rem = n_bits % 8
    bits = bytearray(stream(b"bits" + salt, n_bits // 8 + 1))
    bits[-1] = (bits[-1] & ((1 << rem) - 1)) | (1 << rem)  # the delimiter bit
    f = stream(b"fields" + salt, 96 + 128 + 96 + 8)
    inner = (236 if kind == 2 else 228).to_bytes(4, "little") + f[96:224] + f[224:320] + (f[320:328] if kind == 2 else b"") + bytes(bits)
    return index.to_bytes(8, "little") + (108).to_bytes(4, "little") + f[:96] + inner


def keys_of(ctx):
    sks = [int.from_bytes(hashlib.sha256(b"bench-objects-var-sk" + i.to_bytes(4, "little")).digest(), "big") % R_ORDER or 1
           for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    if any(ctx.pubkey_table_set(0, pks)):
        raise SystemExit("pubkey table load failed")
    return sks, pks


def build_jobs(ctx, sks, pks, n_jobs, kind, n_bits):
    """-> (PreparedJobs in object form, PreparedJobs in root form, sets per package, message bytes)"""
    from lodestar_amd._native import MsgObject, PkIndices, PreparedJobs
    domain = hashlib.sha256(b"bench-objects-var-domain").digest()
    slots = [(5000 + j).to_bytes(8, "little") for j in range(n_jobs)]
    aggs = [agg_proof(kind, n_bits, j, (j % 8).to_bytes(1, "little")) for j in range(n_jobs)]
    datas = [stream(b"data" + j.to_bytes(4, "little"), 128) for j in range(n_jobs)]
    r_slot = ctx.object_signing_roots(slots, domain)
    r_agg = ctx.object_signing_roots_var(kind, aggs, domain)
    r_data = ctx.object_signing_roots(datas, domain)
    signers = [[(7 * j + k) % N_KEYS for k in range(3)] for j in range(n_jobs)]
    sk, msg = [], []
    for j in range(n_jobs):
        a = (3 * j + 1) % N_KEYS
        sk += [sks[a], sks[a], sum(sks[s] for s in signers[j]) % R_ORDER]
        msg += [r_slot[j], r_agg[j], r_data[j]]
    sigs = ctx.sign(sk, msg)
    obj_jobs, root_jobs = [], []
    for j in range(n_jobs):
        a = (3 * j + 1) % N_KEYS
        ks = [[pks[a]], [pks[a]], PkIndices(signers[j])]
        ms = [MsgObject(slots[j], domain), MsgObject(aggs[j], domain, kind), MsgObject(datas[j], domain)]
        obj_jobs.append(([(ks[k], ms[k], sigs[3 * j + k]) for k in range(3)], 1))
        root_jobs.append(([(ks[k], msg[3 * j + k], sigs[3 * j + k]) for k in range(3)], 1))
    msg_bytes = sum(len(m) for job in obj_jobs for _, m, _ in job[0])
    return PreparedJobs(obj_jobs), PreparedJobs(root_jobs), 3 * n_jobs, msg_bytes


def run_leg(ctx, form, pj, n_sets, seconds, depth, min_packages=0):
    lat, sub, flight, done = [], [], [], 0
    t0 = time.perf_counter()
    while True:
        more = time.perf_counter() - t0 < seconds or done + len(flight) < min_packages
        if more and len(flight) < depth:
            ts = time.perf_counter()
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
    return {"form": form, "packages": done, "seconds": round(dt, 3), "sets_per_s": round(done * n_sets / dt, 1),
            "p50_ms": round(1e3 * statistics.median(lat), 3), "submit_us": int(statistics.median(sub))}


def kernel_time(ctx, pj, name, reps=5):
    """median milliseconds of kernel `name` over `reps` synchronous packages"""
    ms = []
    for _ in range(reps + 1):
        res, _ = ctx.verify_jobs(pj)
        if any(r[0] != 1 for r in res):
            raise SystemExit("a package did not verify")
        t = [v for k, v in ctx.last_kernel_times() if k == name]
        if len(t) != 1:
            raise SystemExit(f"{name} did not run exactly once")
        ms.append(t[0])
    return statistics.median(ms[1:])  # (the first package sizes the buffers)


def kernel_alone(ctx, sks, pks):
    from lodestar_amd._native import MsgObject, PreparedJobs
    domain = hashlib.sha256(b"bench-objects-var-domain").digest()
    for n in (128, 8192):
        sk = [sks[i % N_KEYS] for i in range(n)]
        pk = [[pks[i % N_KEYS]] for i in range(n)]
        for kind, n_bits in SHAPES:
            objs = [agg_proof(kind, n_bits, i, (i % 8).to_bytes(1, "little")) for i in range(n)]
            sigs = ctx.sign(sk, ctx.object_signing_roots_var(kind, objs, domain))
            pj = PreparedJobs([([(pk[i], MsgObject(objs[i], domain, kind), sigs[i])], 1) for i in range(n)])
            print(json.dumps({"kernel": "k_msg_roots_var", "kind": kind, "bits": n_bits, "objects": n,
                              "median_us": round(1e3 * kernel_time(ctx, pj, "k_msg_roots_var"), 2)}), flush=True)
            del pj, objs
        datas = [stream(b"alone" + i.to_bytes(4, "little"), 128) for i in range(n)]
        sigs = ctx.sign(sk, ctx.object_signing_roots(datas, domain))
        pj = PreparedJobs([([(pk[i], MsgObject(datas[i], domain), sigs[i])], 1) for i in range(n)])
        print(json.dumps({"kernel": "k_msg_roots", "object": "AttestationData", "objects": n,
                          "median_us": round(1e3 * kernel_time(ctx, pj, "k_msg_roots"), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=256, help="aggregate jobs per package (three sets each)")
    ap.add_argument("--kind", type=int, default=2, help="1: phase0.AggregateAndProof, 2: EIP-7549's")
    ap.add_argument("--bits", type=int, default=28800, help="aggregation bits per aggregate")
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rounds", type=int, default=2, help="object / roots alternations")
    ap.add_argument("--depth", type=int, default=4, help="packages in flight")
    ap.add_argument("--no-kernel", action="store_true", help="skip the kernel-alone packages")
    args = ap.parse_args()
    from lodestar_amd._native import Context
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    t0 = time.perf_counter()
    sks, pks = keys_of(ctx)
    pj_obj, pj_root, n_sets, msg_bytes = build_jobs(ctx, sks, pks, args.jobs, args.kind, args.bits)
    print(f"inputs built in {time.perf_counter() - t0:.1f} s: {n_sets} sets, {msg_bytes} message bytes per package", file=sys.stderr)
    ctx.reserve(n_sets, max_pks=5 * args.jobs, max_msg_bytes=msg_bytes, n_slots=args.depth)
    legs = {"object": pj_obj, "roots": pj_root}
    for form, pj in legs.items():  # warm-up
        run_leg(ctx, form, pj, n_sets, 0.0, args.depth, min_packages=3)
    rate = {"object": [], "roots": []}
    p50 = {"object": [], "roots": []}
    for rnd in range(args.rounds):
        for form, pj in legs.items():
            r = run_leg(ctx, form, pj, n_sets, args.seconds, args.depth)
            r.update({"round": rnd, "sets_per_package": n_sets, "jobs": args.jobs, "kind": args.kind, "bits": args.bits, "depth": args.depth})
            rate[form].append(r["sets_per_s"])
            p50[form].append(r["p50_ms"])
            print(json.dumps(r), flush=True)
    for form, pj in legs.items():  # one package at a time: the latency of a lone package
        r = run_leg(ctx, form, pj, n_sets, args.seconds / 2, 1)
        r.update({"round": "lone", "sets_per_package": n_sets, "depth": 1})
        print(json.dumps(r), flush=True)
    mo, mr = statistics.mean(rate["object"]), statistics.mean(rate["roots"])
    spread = lambda v: round((max(v) - min(v)) / statistics.mean(v), 4)  # noqa: E731
    print(json.dumps({"summary": True, "object_sets_per_s": rate["object"], "roots_sets_per_s": rate["roots"],
                      "object_over_roots": round(mo / mr, 4), "object_leg_spread": spread(rate["object"]),
                      "roots_leg_spread": spread(rate["roots"]), "object_inside_roots_range": min(rate["roots"]) <= mo <= max(rate["roots"]),
                      "object_p50_ms": p50["object"], "roots_p50_ms": p50["roots"]}), flush=True)
    if not args.no_kernel:
        kernel_alone(ctx, sks, pks)
    ctx.close()


if __name__ == "__main__":
    main()
