#!/usr/bin/env python3
"""Block-body packages (bench.py's config C shape) by index list against by committee + bits
(LSG_PK_BITS): 64 blocks per package, each one non-batchable job of 128
aggregate sets, every set a committee of ~450 validators drawn from a 2^20-row pubkey table,
at 99 %, 90 % and 50 % participation.  The same packages run in both forms, alternating in one
process, after a warm-up; a leg runs for at least --seconds and ends with every package waited on
(the device idle).

One JSON line per leg: sets/s, p50 package latency, median submit_us, and the bytes staged per
package for the sets' keys (computed from the shapes: 8 bytes per key by index -- the index
and its length word -- against the bit arena plus the plan words by bits).  A summary line per
participation gives the ratio bits / index.

  python tools/bench_committees.py [--blocks 64] [--seconds 2] [--participation 0.99,0.9,0.5]
  python tools/bench_committees.py --kernel-trace DIR     kernel times per package instead: runs
      itself under `rocprofv3 --kernel-trace --stats` (a run of its own) and prints the time of
      k_pk_agg_seg (index legs) and k_pk_agg_bits (bits legs) per package from the trace
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_KEYS = 1024
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PER_BLOCK = 128


def build(ctx, blocks, validators, participation, seed=1):
    """-> {q: {"index": PreparedJobs, "bits": PreparedJobs, "shape": [(n, p)]}} over one set of
    committees registered as ids 0 .. blocks * 128 - 1"""
    import hashlib
    from lodestar_amd._native import PkBits, PkIndices, PreparedJobs
    sks = [int.from_bytes(hashlib.sha256(b"bench-committees-sk" + i.to_bytes(4, "little")).digest(), "big") % R_ORDER or 1
           for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    if any(ctx.pubkey_table_set(0, [pks[v % N_KEYS] for v in range(validators)])):
        raise SystemExit("pubkey table load failed")
    import numpy as np
    n_sets = blocks * PER_BLOCK
    # (drawn with replacement: a rare repeated member is allowed, as in a sync committee)
    committees = [np.random.default_rng(seed * 1000003 + g).integers(0, validators, 440 + (g * 7) % 21, dtype=np.uint32)
                  for g in range(n_sets)]
    if any(ctx.committees_set(0, [c.tolist() for c in committees])):
        raise SystemExit("committee registration failed")
    msgs = [hashlib.sha256(b"bench-committees-msg" + g.to_bytes(8, "little")).digest() for g in range(n_sets)]
    out = {}
    for q in participation:
        rng = np.random.default_rng(int(q * 1000) + seed)
        by_index, by_bits, agg, shape = [], [], [], []
        for g, members in enumerate(committees):
            n = len(members)
            bits = rng.random(n) < q
            if not bits.any():
                bits[0] = True
            part = members[bits].tolist()
            by_index.append(PkIndices(part))
            by_bits.append(PkBits(g, np.packbits(bits, bitorder="little").tobytes(), n))
            agg.append(sum(sks[v % N_KEYS] for v in part) % R_ORDER)
            shape.append((n, len(part)))
        sigs = ctx.sign(agg, msgs)

        def jobs(keys):
            return [([(keys[b * PER_BLOCK + i], msgs[b * PER_BLOCK + i], sigs[b * PER_BLOCK + i]) for i in range(PER_BLOCK)], 0)
                    for b in range(blocks)]
        out[q] = {"index": PreparedJobs(jobs(by_index)), "bits": PreparedJobs(jobs(by_bits)), "shape": shape}
    return out


def staged_key_bytes(shape):
    """bytes staged per package for the sets' keys, from the shapes (lsg_stage.hpp stage_fill,
    lsg_plan.hpp plan_bits): by index, 4 bytes of index and a 4-byte length word per participant;
    by bits, the field's words plus 6 plan words and one pair-table word per lane pair"""
    index = sum(8 * p for _, p in shape)
    wanted = [n - p if (n - p) + 1 < p else p for n, p in shape]

    def pairs(w, fold):
        lg = 0
        while lg < 5 and (fold << lg) < w:
            lg += 1
        return 1 << lg
    fold = 4
    while sum(pairs(w, fold) for w in wanted) > 131072 and fold < 64:
        fold *= 2
    bits = sum(4 * ((n + 31) // 32) + 4 * (6 + pairs(w, fold)) for (n, _), w in zip(shape, wanted))
    return index, bits


def run_leg(ctx, pj, n_sets, seconds, depth, min_packages=0):
    """packages of `pj` back to back, `depth` in flight, for at least `seconds`"""
    # (no package is in flight on entry; on exit every one has been waited on, and a wait blocks on
    # the completion event recorded behind the package's last kernel and copy: the device is idle)
    lat, sub, flight, done = [], [], [], 0
    t0 = time.perf_counter()
    while True:
        now = time.perf_counter()
        more = now - t0 < seconds or done + len(flight) < min_packages
        if more and len(flight) < depth:
            t = ctx.submit_jobs(pj)
            if t is not None:
                flight.append((t, time.perf_counter()))
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
    return {"packages": done, "seconds": round(dt, 3), "sets_per_s": round(done * n_sets / dt, 1),
            "p50_ms": round(1e3 * statistics.median(lat), 3), "submit_us": int(statistics.median(sub))}


def trace_child(args):
    """under rocprofv3: per participation, --trace-packages packages by index, then as many by bits"""
    from lodestar_amd._native import Context
    ctx = Context(0)
    data = build(ctx, args.blocks, args.validators, args.participation)
    n_sets = args.blocks * PER_BLOCK
    ctx.reserve(n_sets, max_pks=480 * n_sets, n_slots=args.depth)
    for q in args.participation:
        for form in ("index", "bits"):
            run_leg(ctx, data[q][form], n_sets, 0.0, 1, min_packages=args.trace_packages)
    ctx.close()


def kernel_trace(args):
    out = os.path.abspath(args.kernel_trace)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "committees", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", "--blocks", str(args.blocks), "--validators", str(args.validators),
           "--participation", ",".join(str(q) for q in args.participation), "--trace-packages", str(args.trace_packages)]
    subprocess.check_call(cmd)
    dbs = glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise SystemExit("no rocprofv3 database under " + out)
    c = sqlite3.connect(dbs[0])
    rows = c.execute("select name, count(*), sum(end - start), avg(end - start) from kernels "
                     "where name like '%k_pk_agg_%' group by name").fetchall()
    legs = len(args.participation) * args.trace_packages
    for name, calls, total, avg in rows:
        print(json.dumps({"kernel": name.split("(")[0], "calls": calls, "total_ms": round(total * 1e-6, 3),
                          "avg_us": round(avg * 1e-3, 2), "ms_per_package_over_all_legs": round(total * 1e-6 / legs, 4)}))
    # per launch, in launch order: the legs are index, bits per participation
    seq = c.execute("select name, end - start from kernels where name like '%k_pk_agg_%' order by start").fetchall()
    extra = len(seq) - 2 * legs  # (the registration's own aggregation pass comes first)
    if extra < 0:
        raise SystemExit("fewer aggregation launches in the trace than packages")
    seq = seq[extra:]
    per, k = {}, 0
    for q in args.participation:
        for form, kern in (("index", "k_pk_agg_seg"), ("bits", "k_pk_agg_bits")):
            mine = [d for name, d in seq[k:k + args.trace_packages] if kern in name]
            if len(mine) != args.trace_packages:
                raise SystemExit(f"trace does not line up with the legs at {q} {form}")
            per[(q, form)] = statistics.median(mine) * 1e-3
            k += args.trace_packages
    for q in args.participation:
        a, b = per[(q, "index")], per[(q, "bits")]
        print(json.dumps({"participation": q, "k_pk_agg_seg_us_per_package": round(a, 1),
                          "k_pk_agg_bits_us_per_package": round(b, 1), "bits_over_index": round(b / a, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--participation", default="0.99,0.9,0.5")
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rounds", type=int, default=2, help="index / bits alternations per participation")
    ap.add_argument("--depth", type=int, default=4, help="packages in flight")
    ap.add_argument("--kernel-trace", metavar="DIR", default=None)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-packages", type=int, default=10)
    args = ap.parse_args()
    args.participation = [float(x) for x in args.participation.split(",")]
    if args.trace_child:
        return trace_child(args)
    if args.kernel_trace:
        return kernel_trace(args)
    from lodestar_amd._native import Context
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    t0 = time.perf_counter()
    data = build(ctx, args.blocks, args.validators, args.participation)
    n_sets = args.blocks * PER_BLOCK
    print(f"inputs built in {time.perf_counter() - t0:.1f} s: {n_sets} sets per package", file=sys.stderr)
    ctx.reserve(n_sets, max_pks=480 * n_sets, n_slots=args.depth)
    for q in args.participation:  # warm-up: every shape the timed legs use
        for form in ("index", "bits"):
            run_leg(ctx, data[q][form], n_sets, 0.0, args.depth, min_packages=3)
    for q in args.participation:
        ib, bb = staged_key_bytes(data[q]["shape"])
        rate = {"index": [], "bits": []}
        for rnd in range(args.rounds):
            for form in ("index", "bits"):
                r = run_leg(ctx, data[q][form], n_sets, args.seconds, args.depth)
                r.update({"form": form, "participation": q, "round": rnd, "sets_per_package": n_sets,
                          "staged_key_bytes_per_package": ib if form == "index" else bb})
                rate[form].append(r["sets_per_s"])
                print(json.dumps(r), flush=True)
        mi, mb = statistics.mean(rate["index"]), statistics.mean(rate["bits"])
        print(json.dumps({"summary": True, "participation": q, "index_sets_per_s": round(mi, 1), "bits_sets_per_s": round(mb, 1),
                          "bits_over_index": round(mb / mi, 4), "index_rounds": rate["index"], "bits_rounds": rate["bits"],
                          "staged_key_bytes_index": ib, "staged_key_bytes_bits": bb}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
