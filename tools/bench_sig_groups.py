#!/usr/bin/env python3
"""Firehose-shaped packages with and without per-group signature aggregates:
32,768 single-set batchable jobs over 64 committee-shaped messages (512 signers each), one
group per message.  Three routes, alternating in one process after a warm-up, at 1 and 4
packages in flight; a leg runs for at least --seconds and ends with every package waited on
(the device idle):

  plain         lsg_submit_jobs / lsg_wait_jobs: what the verifier does without groups
  grouped       lsg_submit_jobs_grouped / lsg_wait_jobs_grouped: the aggregates come back with
                the verdicts
  plain+agg     plain, then lsg_aggregate_signatures over the package's signatures after each
                wait: a blocking side call that stages and decodes them again

One JSON line per leg: sets/s, p50 package latency, median submit_us and, for grouped legs, the
median time of k_sig_agg_seg from lsg_last_kernel_times.  A summary line per depth gives each
route's rounds, plain's own lowest-to-highest range and the ratios.  --forged adds a plain and
a grouped leg whose packages carry 1 % forged sets (grouped: the sums are planned again over
the sets that verified and launched a second time).

  python tools/bench_sig_groups.py [--sets 32768] [--messages 64] [--seconds 2] [--rounds 2] [--forged]
"""
import argparse
import ctypes
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
B = 1  # LSG_JOB_BATCHABLE


def build(ctx, n_sets, n_msgs, forged_share):
    """-> (PreparedJobs valid, PreparedJobs with forged sets, group ids, the signatures' bytes,
    group offsets for lsg_aggregate_signatures (sets sorted by group), forged count)"""
    from lodestar_amd._native import PreparedJobs
    sks = [int.from_bytes(hashlib.sha256(b"bench-groups-sk" + i.to_bytes(4, "little")).digest(), "big") % R_ORDER or 1
           for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    msgs = [hashlib.sha256(b"bench-groups-msg" + g.to_bytes(8, "little")).digest() for g in range(n_msgs)]
    group = [i % n_msgs for i in range(n_sets)]
    sigs = ctx.sign([sks[i % N_KEYS] for i in range(n_sets)], [msgs[g] for g in group])
    sets = [([pks[i % N_KEYS]], msgs[group[i]], sigs[i]) for i in range(n_sets)]
    good = PreparedJobs([([s], B) for s in sets])
    step = max(1, int(round(1 / forged_share))) if forged_share > 0 else 0
    n_forged = 0
    bad = list(sets)
    for i in range(0, n_sets if step else 0, step or 1):  # a signature over another message of the package
        bad[i] = (bad[i][0], msgs[(group[i] + 1) % n_msgs], bad[i][2])
        n_forged += 1
    forged = PreparedJobs([([s], B) for s in bad]) if step else None
    by_group = sorted(range(n_sets), key=lambda i: group[i])
    flat = b"".join(sigs[i] for i in by_group)
    offs = (ctypes.c_uint32 * (n_msgs + 1))()
    for g in group:
        offs[g + 1] += 1
    for g in range(n_msgs):
        offs[g + 1] += offs[g]
    return good, forged, (ctypes.c_uint32 * n_sets)(*group), flat, offs, n_forged


class Runner:
    def __init__(self, ctx, n_sets, n_groups, ids, flat, offs):
        from lodestar_amd._native import LsgJobResult, LsgStats
        self.ctx, self.lib, self.n_sets, self.ng, self.ids, self.flat, self.offs = ctx, ctx.lib, n_sets, n_groups, ids, flat, offs
        self.res = (LsgJobResult * n_sets)()
        self.st = LsgStats()
        self.agg = ctypes.create_string_buffer(96 * n_groups)
        self.cnt = (ctypes.c_uint32 * n_groups)()
        self.side_out = ctypes.create_string_buffer(96 * n_groups)
        self.side_err = (ctypes.c_int32 * n_groups)()

    def submit(self, pj, route):
        t = ctypes.c_uint64()
        if route == "grouped":
            rc = self.lib.lsg_submit_jobs_grouped(self.ctx.h, pj.jobs, pj.n_jobs, 0, self.ids, self.ng, ctypes.byref(t))
        else:
            rc = self.lib.lsg_submit_jobs(self.ctx.h, pj.jobs, pj.n_jobs, 0, ctypes.byref(t))
        if rc == 6:  # LSG_ERR_BUSY
            return None
        self.ctx._check(rc, "submit")
        return t.value

    def wait(self, t, route):
        if route == "grouped":
            rc = self.lib.lsg_wait_jobs_grouped(self.ctx.h, t, self.res, ctypes.byref(self.st), self.agg, self.cnt)
        else:
            rc = self.lib.lsg_wait_jobs(self.ctx.h, t, self.res, ctypes.byref(self.st))
        self.ctx._check(rc, "wait")
        if route == "plain+agg":
            self.ctx._check(self.lib.lsg_aggregate_signatures(self.ctx.h, self.flat, 96, self.offs, self.ng, self.side_out,
                                                               self.side_err), "lsg_aggregate_signatures")

    def leg(self, pj, route, seconds, depth, min_packages=0, expect_valid=None):
        import numpy as np
        lat, sub, kagg, flight, done = [], [], [], [], 0
        status = np.frombuffer(self.res, dtype=np.int32)[::2]
        t0 = time.perf_counter()
        while True:
            more = time.perf_counter() - t0 < seconds or done + len(flight) < min_packages
            if more and len(flight) < depth:
                t = self.submit(pj, route)
                if t is not None:
                    flight.append((t, time.perf_counter()))
                    continue
            if not flight:
                break
            t, ts = flight.pop(0)
            self.wait(t, route)
            lat.append(time.perf_counter() - ts)
            sub.append(self.st.submit_us)
            valid = int((status == 1).sum())
            if expect_valid is not None and valid != expect_valid:
                raise SystemExit(f"{route}: {valid} valid jobs, expected {expect_valid}")
            if route == "grouped":
                if sum(self.cnt) != valid:
                    raise SystemExit(f"grouped: {sum(self.cnt)} signatures summed, {valid} valid jobs")
                if done % 8 == 0:  # (a side call of its own: sampled)
                    kagg.append(sum(ms for name, ms in self.ctx.last_kernel_times() if name == "k_sig_agg_seg"))
            done += 1
        dt = time.perf_counter() - t0
        out = {"route": route, "depth": depth, "packages": done, "seconds": round(dt, 3),
               "sets_per_s": round(done * self.n_sets / dt, 1), "p50_ms": round(1e3 * statistics.median(lat), 3),
               "submit_us": int(statistics.median(sub))}
        if kagg:
            out["k_sig_agg_seg_ms"] = round(statistics.median(kagg), 4)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=32768)
    ap.add_argument("--messages", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the three routes per depth")
    ap.add_argument("--depths", default="1,4", help="packages in flight")
    ap.add_argument("--forged", action="store_true", help="add the legs with 1 %% forged sets")
    args = ap.parse_args()
    depths = [int(x) for x in args.depths.split(",")]
    from lodestar_amd._native import Context
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    t0 = time.perf_counter()
    good, forged, ids, flat, offs, n_forged = build(ctx, args.sets, args.messages, 0.01 if args.forged else 0.0)
    print(f"inputs built in {time.perf_counter() - t0:.1f} s: {args.sets} sets, {args.messages} groups", file=sys.stderr)
    run = Runner(ctx, args.sets, args.messages, ids, flat, offs)
    ctx.reserve(args.sets, n_slots=max(depths))
    run.leg(good, "grouped", 0.0, 1, min_packages=1, expect_valid=args.sets)  # the first grouped package allocates
    ctx.reserve(args.sets, n_slots=max(depths))  # ... and the caller reserves again
    routes = ("plain", "grouped", "plain+agg")
    for route in routes:  # warm-up: every route at the largest depth
        run.leg(good, route, 0.0, max(depths), min_packages=max(depths) + 2, expect_valid=args.sets)
    for depth in depths:
        rate = {r: [] for r in routes}
        for rnd in range(args.rounds):
            for route in routes:
                r = run.leg(good, route, args.seconds, depth, expect_valid=args.sets)
                r.update({"round": rnd, "sets_per_package": args.sets, "groups": args.messages})
                rate[route].append(r["sets_per_s"])
                print(json.dumps(r), flush=True)
        mean = {r: statistics.mean(rate[r]) for r in routes}
        print(json.dumps({"summary": True, "depth": depth, "rounds": rate,
                          "plain_range": [min(rate["plain"]), max(rate["plain"])],
                          "grouped_over_plain": round(mean["grouped"] / mean["plain"], 4),
                          "grouped_over_plain_agg": round(mean["grouped"] / mean["plain+agg"], 4)}), flush=True)
    if args.forged:
        depth = max(depths)
        for route in ("plain", "grouped"):
            run.leg(forged, route, 0.0, depth, min_packages=depth, expect_valid=args.sets - n_forged)
        for rnd in range(args.rounds):
            for route in ("plain", "grouped"):
                r = run.leg(forged, route, args.seconds, depth, expect_valid=args.sets - n_forged)
                r.update({"round": rnd, "forged_sets": n_forged, "sets_per_package": args.sets, "groups": args.messages})
                print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
