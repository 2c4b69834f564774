#!/usr/bin/env python3
"""Electra block bodies by index list against by committee list + one bitfield
(LSG_PK_BITS_MULTI): 64 blocks per package, each one non-batchable job of 8
aggregate sets, every set spanning the 64 committees of one slot -- 440 to 460 validators each,
drawn from a 2^20-row pubkey table -- at 99 %, 90 % and 50 % participation.  That is 512 sets
of ~28,800 bits, 14.7M bits per package: four times the ~3.7M keys of bench.py's config C,
because 8 aggregates of a whole slot each are more signers than 128 single committees (DESIGN.md
5i).  Block b's set t
attests slot b + t, so a slot's committees serve up to 8 blocks of the package, as they do in a
range of consecutive blocks: (blocks + 7) x 64 committees are registered.

The same packages run in both forms, alternating in one process, after a warm-up; a leg runs
for at least --seconds with --depth packages in flight and ends with every package waited on.

One JSON line per leg: sets/s, keys/s, p50 package latency, median submit_us, a MODEL of the
bytes staged per package for the sets' keys (staged_key_bytes_model_*: not read back from the
library but computed here from the shapes by the rules of stage_fill (lsg_stage.hpp) and plan_multi -- 8 bytes
per key by index, the index and its length word, against the parts' arena words plus the plan
words by committee list),
and the aggregation kernels' time per package from lsg_last_kernel_times (k_pk_agg_seg and its
later passes, listed as g1_aggregate, for the index form; k_pk_agg_bits_multi for the other),
the median over --kernel-packages packages run one at a time after the leg.  A summary line per
participation gives the ratio multi / index.

  python tools/bench_committees_multi.py [--blocks 64] [--seconds 2] [--participation 0.99,0.9,0.5]
"""
import argparse
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
PER_BLOCK = 8
PER_SLOT = 64
AGG_KERNELS = {"index": ("g1_aggregate",), "multi": ("k_pk_agg_bits_multi",)}


def build(ctx, blocks, validators, participation, seed=1):
    """-> {q: {"index": PreparedJobs, "multi": PreparedJobs, "shape": per set [(n, p) per part]}}
    over one set of committees registered as ids 0 .. (blocks + 7) * 64 - 1"""
    import hashlib
    import numpy as np
    from lodestar_amd._native import PkBitsMulti, PkIndices, PreparedJobs
    sks = [int.from_bytes(hashlib.sha256(b"bench-committees-sk" + i.to_bytes(4, "little")).digest(), "big") % R_ORDER or 1
           for i in range(N_KEYS)]
    pks = ctx.sk_to_pk(sks)
    if any(ctx.pubkey_table_set(0, [pks[v % N_KEYS] for v in range(validators)])):
        raise SystemExit("pubkey table load failed")
    n_slots = blocks + PER_BLOCK - 1
    # (drawn with replacement: a rare repeated member is allowed, as in a sync committee)
    committees = [np.random.default_rng(seed * 1000003 + g).integers(0, validators, 440 + (g * 7) % 21, dtype=np.uint32)
                  for g in range(n_slots * PER_SLOT)]
    if any(ctx.committees_set(0, [c.tolist() for c in committees])):
        raise SystemExit("committee registration failed")
    n_sets = blocks * PER_BLOCK
    msgs = [hashlib.sha256(b"bench-committees-multi-msg" + g.to_bytes(8, "little")).digest() for g in range(n_sets)]
    out = {}
    for q in participation:
        rng = np.random.default_rng(int(q * 1000) + seed)
        by_index, by_multi, agg, shape = [], [], [], []
        for g in range(n_sets):
            slot = g // PER_BLOCK + g % PER_BLOCK
            ids = list(range(slot * PER_SLOT, (slot + 1) * PER_SLOT))
            members = np.concatenate([committees[c] for c in ids])
            bits = rng.random(len(members)) < q
            if not bits.any():
                bits[0] = True
            part = members[bits]
            by_index.append(PkIndices(part.tolist()))
            by_multi.append(PkBitsMulti(ids, np.packbits(bits, bitorder="little").tobytes(), len(members)))
            counts = np.bincount(part % N_KEYS, minlength=N_KEYS)
            agg.append(sum(int(n) * sk for n, sk in zip(counts, sks) if n) % R_ORDER)
            off, parts = 0, []
            for c in ids:
                n = len(committees[c])
                parts.append((n, int(bits[off:off + n].sum())))
                off += n
            shape.append(parts)
        sigs = ctx.sign(agg, msgs)

        def jobs(keys):
            return [([(keys[b * PER_BLOCK + i], msgs[b * PER_BLOCK + i], sigs[b * PER_BLOCK + i]) for i in range(PER_BLOCK)], 0)
                    for b in range(blocks)]
        out[q] = {"index": PreparedJobs(jobs(by_index)), "multi": PreparedJobs(jobs(by_multi)), "shape": shape}
    return out


def reserve_units(shape):
    """what the package's multi sets count toward lsg_reserve's max_pks (include/lodestar_bls.h)"""
    return sum(16 + 2 * len(parts) + (sum(n for n, _ in parts) + 31) // 32 for parts in shape)


def staged_key_bytes(shape):
    """a model of the bytes staged per package for the sets' keys, from the shapes (lsg_stage.hpp stage_fill,
    lsg_plan.hpp plan_multi): by index, 4 bytes of index and a 4-byte length word per
    participant; by committee list, the words of every part with a participant plus 5 plan
    words per set, 4 per part and one pair-table word per lane pair"""
    index = sum(8 * p for parts in shape for _, p in parts)
    items = [sum((n - p + 1 if (n - p) + 1 < p else p) for n, p in parts if p) for parts in shape]

    def pairs(w, fold):
        lg = 0
        while lg < 5 and (fold << lg) < w:
            lg += 1
        return 1 << lg
    fold = 4
    while sum(pairs(w, fold) for w in items) > 131072 and fold < 64:
        fold *= 2
    multi = sum(sum(4 * ((n + 31) // 32) + 16 for n, p in parts if p) + 4 * (5 + pairs(w, fold))
                for parts, w in zip(shape, items))
    return index, multi


def run_leg(ctx, pj, n_sets, n_keys, seconds, depth, min_packages=0):
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
            "keys_per_s": round(done * n_keys / dt, 1), "p50_ms": round(1e3 * statistics.median(lat), 3),
            "submit_us": int(statistics.median(sub))}


def kernel_us(ctx, pj, form, packages):
    """the aggregation kernels' time per package (lsg_last_kernel_times), one package at a time"""
    per = []
    for _ in range(packages):
        res, _st = ctx.wait_jobs(ctx.submit_jobs(pj), raw=True)
        if any(res[j].status != 1 for j in range(pj.n_jobs)):
            raise SystemExit("a package did not verify")
        times = ctx.last_kernel_times()
        other = [k for k, _ in times if k.startswith("k_pk_agg") or k == "g1_aggregate"]
        if not other or any(k not in AGG_KERNELS[form] for k in other):
            raise SystemExit(f"{form} package launched {sorted(set(other))}")
        per.append(1e3 * sum(ms for k, ms in times if k in AGG_KERNELS[form]))
    return round(statistics.median(per), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--participation", default="0.99,0.9,0.5")
    ap.add_argument("--seconds", type=float, default=2.0, help="least time per leg")
    ap.add_argument("--rounds", type=int, default=2, help="index / multi alternations per participation")
    ap.add_argument("--depth", type=int, default=4, help="packages in flight")
    ap.add_argument("--kernel-packages", type=int, default=5)
    args = ap.parse_args()
    args.participation = [float(x) for x in args.participation.split(",")]
    from lodestar_amd._native import Context
    ctx = Context(0)  # raises without a gfx950 device: there is no CPU path to time
    t0 = time.perf_counter()
    data = build(ctx, args.blocks, args.validators, args.participation)
    n_sets = args.blocks * PER_BLOCK
    print(f"inputs built in {time.perf_counter() - t0:.1f} s: {n_sets} sets per package", file=sys.stderr)
    units = max(reserve_units(d["shape"]) for d in data.values())
    keys = {q: sum(p for parts in data[q]["shape"] for _, p in parts) for q in args.participation}
    ctx.reserve(n_sets, max_pks=max(max(keys.values()), units), n_slots=args.depth)
    for q in args.participation:  # warm-up: every shape the timed legs use
        for form in ("index", "multi"):
            run_leg(ctx, data[q][form], n_sets, keys[q], 0.0, args.depth, min_packages=3)
    for q in args.participation:
        ib, mb = staged_key_bytes(data[q]["shape"])
        rate = {"index": [], "multi": []}
        kern = {}
        for rnd in range(args.rounds):
            for form in ("index", "multi"):
                r = run_leg(ctx, data[q][form], n_sets, keys[q], args.seconds, args.depth)
                kern[form] = kernel_us(ctx, data[q][form], form, args.kernel_packages)
                r.update({"form": form, "participation": q, "round": rnd, "sets_per_package": n_sets,
                          "keys_per_package": keys[q], "staged_key_bytes_model_per_package": ib if form == "index" else mb,
                          "agg_kernels_us_per_package": kern[form]})
                rate[form].append(r["sets_per_s"])
                print(json.dumps(r), flush=True)
        mi, mm = statistics.mean(rate["index"]), statistics.mean(rate["multi"])
        print(json.dumps({"summary": True, "participation": q, "index_sets_per_s": round(mi, 1), "multi_sets_per_s": round(mm, 1),
                          "multi_over_index": round(mm / mi, 4), "index_rounds": rate["index"], "multi_rounds": rate["multi"],
                          "staged_key_bytes_model_index": ib, "staged_key_bytes_model_multi": mb,
                          "agg_kernels_us_index": kern["index"], "agg_kernels_us_multi": kern["multi"]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
