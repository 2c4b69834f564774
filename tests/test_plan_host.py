"""The host-only policy of the verifier (lodestar_amd/csrc/lsg_plan.hpp) on the CPU, through the
stand-alone driver tests/native/plancheck.cpp built with AddressSanitizer and UBSan.

a) Verdict parity: packages of jobs with abstract per-set outcomes go through plan_groups ->
   plan_phase -> resolve_package with a fake group check (a group passes iff each of its sets
   without an error is valid).  Expected verdicts and counters are the oracle's own
   verify_many_signature_sets (chunking, retry, error order, both counters) with its four crypto
   entry points looking the abstract outcomes up.
b) Plan invariants: the driver executes every planned reduction on 64-bit integers and compares
   with the direct sums (plan_seg cases here; plan_phase's items, products and bucket MSM for
   phase A and every fallback phase of every package of a)).
"""
import os
import random
import shutil
import subprocess

import pytest

from oracle import verifier as V
from oracle.curves import BlstError, BLST_NAMES, BLST_PK_IS_INFINITY

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "plancheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

BATCHABLE, VALIDATE_KEYS = 1, 4  # LSG_JOB_* (include/lodestar_bls.h)
VALID, INVALID, ERROR = 1, 0, 2  # LSG_VALID / LSG_INVALID / LSG_ERROR
ERR_EMPTY_SET, ERR_EMPTY_AGGREGATE = 100, 101
CODES = {"BLST_ERROR: " + name: code for code, name in BLST_NAMES.items()}
CODES.update({"Empty signature set": ERR_EMPTY_SET, "EMPTY_AGGREGATE_ARRAY": ERR_EMPTY_AGGREGATE})
SWITCHES = dict(K=4, msm_min=256, package_group=1, sub_groups=1, nb_merge=1, b0_min=64, b0_run=4, lone_ok=1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plancheck") / "plancheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_hostcheck_math.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("plancheck_cases")
    count = [0]

    def run(ints, n_cases):
        count[0] += 1
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in [n_cases] + ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"plancheck exit {p.returncode}: {p.stderr[-2000:]}"
        with open(out) as fh:
            lines = fh.read().splitlines()
        assert len(lines) == n_cases
        return lines
    return run


# ---------------------------------------------------------------- packages and their oracle
def S(valid=True, sig_err=0, pinf=0, keys=(0,)):
    """one set: its abstract outcome, and per key a decode error (keys=(): no keys)"""
    return dict(valid=valid, sig_err=sig_err, pinf=pinf, keys=tuple(keys))


def J(sets, batchable=True, validate=False):
    return dict(sets=list(sets), batchable=batchable, validate=validate)


def singles(n, bad=(), **kw):
    """n batchable single-set jobs, those at `bad` invalid"""
    return [J([S(valid=i not in bad)], **kw) for i in range(n)]


def mixed(n, bad=(), thrown=(), **kw):
    """n batchable jobs of 1, 2, 3, 1, ... sets; `bad` / `thrown`: set numbers (package order)
    that are invalid / whose signature does not decode"""
    jobs, i = [], 0
    for j in range(n):
        sets = []
        for _ in range(1 + j % 3):
            sets.append(S(valid=i not in bad, sig_err=3 if i in thrown else 0))
            i += 1
        jobs.append(J(sets, **kw))
    return jobs


class Tok:
    """what stands for a set's key and signature bytes in the oracle's work requests"""

    def __init__(self, job, s, validate):
        self.job, self.s = job, s
        self.kv = validate and len(s["keys"]) > 0  # its keys are validated: a bad one fails the set
        self.key_err = next((e for e in s["keys"] if e), 0)


@pytest.fixture(autouse=True)
def abstract_crypto(monkeypatch):
    """the oracle's crypto entry points look the abstract outcomes up"""
    def public_key_from_bytes(t):
        if t.key_err and not t.kv:
            Tok.thrown_job = t.job
            raise BlstError(t.key_err)
        return t

    def signature_from_bytes(t, validate=True):
        if t.kv and t.key_err:  # inside a set the key's code beats the signature's
            raise BlstError(t.key_err)
        if t.s["sig_err"]:
            raise BlstError(t.s["sig_err"])
        return t

    def check_keys(sets):
        for pk, _, _ in sets:  # (mul_n_aggregate / verify reject a key in set order)
            if not pk.s["keys"]:
                raise ValueError("EMPTY_AGGREGATE_ARRAY")
            if pk.s["pinf"]:
                raise BlstError(BLST_PK_IS_INFINITY)

    def verify_multiple(sets, rands=None):
        check_keys(sets)
        return all(pk.s["valid"] for pk, _, _ in sets)

    def verify_single(pk, msg, sig):
        check_keys([(pk, msg, sig)])
        return bool(pk.s["valid"])

    for f in (public_key_from_bytes, signature_from_bytes, verify_multiple, verify_single):
        monkeypatch.setattr(V, f.__name__, f)


def oracle_package(jobs):
    """one package alone through worker.ts:30-106 -> (per job (status, code), retries, success,
    key_error, key_error_job)"""
    reqs = []
    for j, job in enumerate(jobs):
        toks = [Tok(j, s, job["validate"]) for s in job["sets"]]
        reqs.append({"opts": {"batchable": job["batchable"]},
                     "sets": [{"publicKey": t, "message": b"", "signature": t} for t in toks]})
    try:
        r = V.verify_many_signature_sets(reqs, rand_fn=lambda: 1)
    except BlstError as e:  # deserializeSet: a bad key rejects every job of the package
        return [(ERROR, e.code)] * len(jobs), 0, 0, e.code, Tok.thrown_job
    res = [(VALID if v else INVALID, 0) if kind == "success" else (ERROR, CODES[v]) for kind, v in r["results"]]
    return res, r["batch_retries"], r["batch_sigs_success"], 0, 0


def expected_line(jobs, subs):
    """the driver's line: a coalesced launch equals each sub-package alone, counters per
    sub-package (the launch's own counters are their sums, its key error none)"""
    parts = [jobs] if not subs else [jobs[a:b] for a, b in zip(subs, subs[1:])]
    got = [oracle_package(p) for p in parts]
    out = []
    for res, *_ in got:
        for st, code in res:
            out += ["J", st, code]
    if subs:
        out += ["S", sum(g[1] for g in got), sum(g[2] for g in got), 0, 0]
        for _, retries, success, ke, kj in got:
            out += ["U", retries, success, ke, kj]
    else:
        out += ["S"] + list(got[0][1:])
    return " ".join(str(x) for x in out)


def case_ints(jobs, subs, sw, seed):
    # rnd_mode (chosen phase-A randomizers, plancheck.cpp case kind 3) only where a case names one
    head = [3, sw["rnd_mode"]] if sw.get("rnd_mode") else [1]
    v = [head[0], sw["K"], sw["msm_min"], sw["package_group"], sw["sub_groups"], sw["nb_merge"], sw["b0_min"], sw["b0_run"],
         sw["lone_ok"]] + head[1:] + [seed, len(jobs), len(subs or [])] + list(subs or [])
    for job in jobs:
        v += [(BATCHABLE if job["batchable"] else 0) | (VALIDATE_KEYS if job["validate"] else 0), len(job["sets"])]
        for s in job["sets"]:
            v += [int(s["valid"]), s["sig_err"], s["pinf"], len(s["keys"])] + list(s["keys"])
    return v


def check(driver, cases):
    """cases: (name, jobs, sub bounds or None, switches).  Returns the fallback-phase counts."""
    ints = []
    for k, (_, jobs, subs, sw) in enumerate(cases):
        ints += case_ints(jobs, subs, dict(SWITCHES, **sw), 1000 + k)
    lines = driver(ints, len(cases))
    calls = []
    for (name, jobs, subs, sw), line in zip(cases, lines):
        verdicts, _, n_calls = line.rpartition(" C ")
        assert verdicts.strip() == expected_line(jobs, subs), f"{name} {sw}"
        calls.append(int(n_calls.partition(" P ")[0]))
    return calls


def bucket_passes(driver, cases):
    """check(), and the number of passes of phase A's bucket plan per case (rnd_mode cases)"""
    ints = []
    for k, (_, jobs, subs, sw) in enumerate(cases):
        ints += case_ints(jobs, subs, dict(SWITCHES, **sw), 1000 + k)
    check(driver, cases)
    return [int(line.rpartition(" P ")[2]) for line in driver(ints, len(cases))]


def variants(name, jobs, subs=None, **fixed):
    """the package under every item width, MSM threshold (group order only), phase-A mode,
    merged non-batchable group on and off, scaled and unscaled lone sets"""
    out = []
    for K in (1, 4):
        for msm_min in (1, 256):
            for mode in (1, 0):
                for nb_merge in (1, 0):
                    for lone_ok in (1, 0):
                        sw = dict(K=K, msm_min=msm_min, nb_merge=nb_merge, lone_ok=lone_ok)
                        sw["sub_groups" if subs else "package_group"] = mode
                        sw.update(fixed)
                        out.append((name, jobs, subs, sw))
    return out


# ---------------------------------------------------------------- a) verdict parity
def test_chunk_counts(driver):
    """chunkify splits from 32 batchable jobs up: every count around a boundary, all valid, the
    first / last job invalid, and the middle job's signature undecodable"""
    cases = []
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49):
        cases += variants(f"{n} valid", singles(n))
        if n:
            cases += variants(f"{n} first bad", singles(n, bad={0}))
            cases += variants(f"{n} last bad", singles(n, bad={n - 1}))
            cases += variants(f"{n} mixed sizes, last set bad", mixed(n, bad={sum(1 + j % 3 for j in range(n)) - 1}))
            jobs = singles(n)
            jobs[n // 2]["sets"][0]["sig_err"] = 10
            cases += variants(f"{n} middle thrown", jobs)
    check(driver, cases)


def test_job_shapes(driver):
    """items of four sets crossing job boundaries (C1), zero-set jobs, an all-empty chunk, a
    chunk whose only bad set is thrown, a thrown and an invalid set in one item"""
    cases = []
    for n in (7, 20, 40, 49):
        total = sum(1 + j % 3 for j in range(n))
        for bad in ({0}, {total // 2}, {total - 1}, {1, total // 2, total - 2}):
            cases += variants(f"mixed {n} bad {sorted(bad)}", mixed(n, bad=bad))
        cases += variants(f"mixed {n} thrown only", mixed(n, thrown={total // 2}))
        # the 10^7 soak's C1 case: a thrown and an invalid set in the same four-set item
        cases += variants(f"mixed {n} thrown+bad in one item", mixed(n, bad={5}, thrown={4}))
        cases += variants(f"mixed {n} thrown job's other set bad", mixed(n, bad={2}, thrown={1}))
    for n in (16, 40):
        jobs = singles(n, bad={3})
        jobs[2]["sets"][0]["sig_err"] = 1  # same item as the invalid set (K = 4)
        cases += variants(f"singles {n} thrown+bad in one item", jobs)
        jobs = singles(n)
        jobs[n - 1]["sets"][0]["pinf"] = 1
        cases += variants(f"singles {n} infinite key only", jobs)
        jobs = singles(n, bad={n - 2})
        jobs[0]["sets"][0]["keys"] = ()
        cases += variants(f"singles {n} no keys + bad", jobs)
    # zero-set jobs, batchable and not; an all-empty chunk (jobs 0..15 of 32)
    empty = [J([]) for _ in range(16)]
    cases += variants("all-empty chunk + valid chunk", empty + singles(16))
    cases += variants("all-empty chunk + failing chunk", empty + singles(16, bad={7}))
    cases += variants("only empty batchable jobs", [J([]) for _ in range(3)])
    cases += variants("empty jobs inside a passing chunk", [J([])] + singles(5) + [J([])])
    cases += variants("empty jobs inside a failing chunk", [J([])] + mixed(9, bad={4}) + [J([]), J([], batchable=False)])
    check(driver, cases)


def nonbatchable(n):
    shapes = [[S()], [S(), S(valid=False)], [], [S(), S(sig_err=3), S()], [S(pinf=1)], [S(keys=())], [S(), S()]]
    return [J(shapes[k % len(shapes)], batchable=False) for k in range(n)]


def test_non_batchable_jobs(driver):
    """0, 1, 2 and 5 non-batchable jobs, merged and per job (variants), alone and beside
    batchable chunks; a failing merged group localises per job"""
    cases = []
    for n in (0, 1, 2, 5, 7):
        for batch in ([], singles(3), mixed(20, bad={11})):
            jobs = nonbatchable(n)
            cases += variants(f"{n} non-batchable + {len(batch)} batchable", batch[:2] + jobs + batch[2:])
    good = [J([S(), S()], batchable=False), J([S()], batchable=False), J([S(), S(), S()], batchable=False)]
    cases += variants("merged group passes", good)
    cases += variants("merged group: last job invalid", good + [J([S(valid=False)], batchable=False)])
    check(driver, cases)


def test_validated_and_bad_keys(driver):
    """deserializeSet: the first bad key in caller order rejects the package; a validated key
    fails its set only"""
    cases = []
    jobs = singles(20)
    jobs[7]["sets"][0]["keys"] = (0, 2)
    jobs[12]["sets"][0]["keys"] = (1,)
    cases += variants("bad keys in jobs 7 and 12", jobs)
    jobs = [J([S()], batchable=False), J([S(keys=(3,))], batchable=False)] + singles(4)
    cases += variants("bad key in a non-batchable job staged last", jobs)
    jobs = mixed(20, bad={9})
    jobs[3] = J([S(keys=(0, 3, 1)), S(sig_err=10, keys=(0,))], validate=True)
    jobs[4] = J([S(sig_err=1, keys=(2,))], validate=True)
    cases += variants("validated keys fail their sets", jobs)
    jobs = mixed(20)
    jobs[3] = J([S(keys=(6,))], validate=True)
    jobs[19]["sets"][0]["keys"] = (2,)
    cases += variants("a validated bad key before a package-wide one", jobs)
    jobs = [J([S(keys=(3,))], batchable=False, validate=True), J([S(keys=())], validate=True)] + singles(3)
    cases += variants("validated non-batchable job, validated set without keys", jobs)
    check(driver, cases)


def test_coalesced_sub_packages(driver):
    """2 and 3 sub-packages, one group per sub-package and per chunk: each equals the
    sub-package run alone; a sub-package of exactly one chunk, of one set, with a bad key"""
    one_chunk = singles(20, bad={13})
    one_set = [J([S()])]
    one_bad_set = [J([S(valid=False)])]
    two_chunks = mixed(33, bad={30}, thrown={3})
    bad_key = singles(5)
    bad_key[2]["sets"][0]["keys"] = (1,)
    nb_only = [J([S(), S()], batchable=False)]
    combos = [[one_chunk, one_set], [one_set, one_chunk], [one_bad_set, two_chunks], [one_chunk, one_set, two_chunks],
              [two_chunks, bad_key, one_chunk], [nb_only, one_chunk, one_bad_set], [singles(16), singles(32, bad={31})],
              [[J([])], one_set, singles(17)], [mixed(40, bad={0, 70}), mixed(48)]]
    cases = []
    for subs in combos:
        jobs, bounds = [], [0]
        for p in subs:
            jobs += p
            bounds.append(len(jobs))
        cases += variants(f"coalesced {[len(p) for p in subs]}", jobs, bounds, b0_min=64)
        cases += variants(f"coalesced {[len(p) for p in subs]} B0 from 2", jobs, bounds, b0_min=2, b0_run=2)
    check(driver, cases)


def test_phase_b0_default_threshold(driver):
    """64 chunks to check reach phase B0, 63 do not; bad sets at the first and last position of
    a run of four chunks; 65 chunks leave a last run of one"""
    cases, want_b0 = [], []
    for n_chunks in (63, 64, 65):
        n = 16 * n_chunks
        for bad in ({0}, {63}, {64, n - 1}, {n - 16}, {5, 200, 777}):
            for K in (1, 4):
                cases.append((f"{n_chunks} chunks bad {sorted(bad)}", singles(n, bad=bad), None, dict(K=K, msm_min=256)))
                want_b0.append(n_chunks >= 64)
    cases.append(("65 chunks of mixed jobs", mixed(1040, bad={1, 1000}, thrown={500}), None, dict(msm_min=1)))
    want_b0.append(True)
    calls = check(driver, cases)
    for (name, _, _, sw), n_calls, b0 in zip(cases, calls, want_b0):
        if "mixed" not in name:  # B0 adds one phase to B and C1; one-job C1 groups (K = 1) need no C2
            assert n_calls == int(b0) + 2 + (sw["K"] == 4), f"{name} {sw}"


def test_phase_b0_lowered_threshold(driver):
    """threshold 2, runs of 2 and 4 over 4 to 9 chunks: one bad set at the first and at the last
    position of every run, the last, shorter run included"""
    cases = []
    for n_chunks in range(4, 10):
        for run in (2, 4):
            for r0 in range(0, n_chunks, run):
                r1 = min(n_chunks, r0 + run)
                for K in (1, 4):
                    sw = dict(K=K, b0_min=2, b0_run=run)
                    for bad in (16 * r0, 16 * r1 - 1):
                        cases.append((f"{n_chunks} chunks run {run} bad {bad}", singles(16 * n_chunks, bad={bad}), None, sw))
            jobs = mixed(16 * n_chunks, bad={0, 31 * n_chunks}, thrown={17})
            cases += variants(f"{n_chunks} chunks of mixed jobs run {run}", jobs, b0_min=2, b0_run=run)
    check(driver, cases)


RND_MODES = {"all equal": 1, "single bit": 2, "all ones": 3, "one window": 4}


def test_skewed_randomizers(driver):
    """Chosen phase-A randomizers (tests/test_gpu_rlc_edges.py runs the same patterns on the
    device) at 256, 513 and 600 single-set jobs: buckets that hold every set -- past 512 members
    (32 lane pairs x 16 folds) the bucket plan takes a second pass -- and bit sums over empty
    buckets only, executed on integers; valid packages and ones whose fallback phases run"""
    cases = []
    for n in (256, 513, 600):
        for mode in RND_MODES.values():
            for K in (1, 4):
                for msm_min in (1, 256):
                    sw = dict(K=K, msm_min=msm_min, rnd_mode=mode)
                    cases.append((f"{n} valid", singles(n), None, sw))
                    cases.append((f"{n} two bad", singles(n, bad={3, n - 1}), None, sw))
            cases.append((f"{n} mixed", mixed(n // 2, bad={n // 3}, thrown={7}), None, dict(msm_min=1, rnd_mode=mode)))
    passes = bucket_passes(driver, cases)
    for (name, jobs, _, sw), p in zip(cases, passes):
        n_sets = sum(len(j["sets"]) for j in jobs)
        full = sw["rnd_mode"] != RND_MODES["one window"]  # a bucket holds every set of the group
        assert p == (2 if full and n_sets > 512 else 1), f"{name} {sw}: {p} passes"


def random_package(rng):
    def rset():
        keys = tuple(rng.choice((1, 2, 3)) if rng.random() < 0.004 else 0 for _ in range(rng.choice((1, 1, 1, 2, 3))))
        return S(valid=rng.random() > 0.08, sig_err=rng.choice((1, 3, 10)) if rng.random() < 0.04 else 0,
                 pinf=int(rng.random() < 0.02), keys=() if rng.random() < 0.01 else keys)

    def rjobs(n):
        return [J([rset() for _ in range(rng.choice((0, 1, 1, 1, 2, 3)))], batchable=rng.random() < 0.85,
                  validate=rng.random() < 0.1) for _ in range(n)]
    sw = dict(K=rng.choice((1, 4)), msm_min=rng.choice((1, 2, 256)), package_group=rng.randrange(2),
              sub_groups=rng.randrange(2), nb_merge=rng.randrange(2), b0_min=rng.choice((0, 2, 64)),
              b0_run=rng.choice((2, 3, 4)), lone_ok=rng.randrange(2))
    if rng.random() < 0.3:
        jobs, bounds = [], [0]
        for _ in range(rng.choice((2, 3))):
            jobs += rjobs(rng.choice((0, 1, 2, 17, 33, rng.randrange(40))))
            bounds.append(len(jobs))
        return ("random coalesced", jobs, bounds, sw)
    return ("random", rjobs(rng.choice((rng.randrange(8), rng.randrange(40), rng.randrange(32, 100)))), None, sw)


def test_random_sweep(driver):
    rng = random.Random(20240611)
    check(driver, [random_package(rng) for _ in range(4000)])


# ---------------------------------------------------------------- b) plan_seg
@pytest.mark.parametrize("op,fold", [(0, 16), (1, 16), (2, 4)])
def test_plan_seg_reduces_every_segment_once(driver, op, fold):
    lens = [0, 1, fold, fold + 1, 32 * fold, 32 * fold + 1, 8193]
    ints, n = [], 0
    for has_idx in (0, 1):
        ints += [2, op, 64, has_idx, len(lens)] + [x for l in lens for x in (l, 1)]  # all in one plan
        ints += [2, op, 64, has_idx, 2, 3, 40, 8193, 1]  # many short segments and a long one
        n += 2
        for l in lens:  # each alone: the mean length sets the lane pairs per chunk
            ints += [2, op, 64, has_idx, 1, l, 1]
            n += 1
    lines = driver(ints, n)
    assert all(line.startswith("seg ok") for line in lines)
    # 8,193 terms alone: 65 partial products of <= 128 (op 2), 17 partial sums of <= 512
    assert lines[-1] == "seg ok passes 2"
    assert lines[2] == "seg ok passes 1"  # an empty segment alone still writes its identity


@pytest.mark.parametrize("wide", [64, 32])
def test_plan_seg_wide_fold(driver, wide):
    """from 4,096 segments (131,072 lane pairs at 32 per segment) a pass folds up to `wide`
    terms per pair on as few pairs as fit the longest segment"""
    lens = [0, 1, wide, wide + 1, 32 * wide, 32 * wide + 1, 8193]
    ints = []
    for has_idx in (0, 1):
        ints += [2, 1, wide, has_idx, len(lens) + 1] + [x for l in lens for x in (l, 1)] + [3, 4096]
        ints += [2, 0, wide, has_idx, 2, wide + 1, 4096, 2 * wide, 1]
    ints += [2, 2, wide, 0, 1, 200, 4096]  # Fp12 products never fold wide: 200 > 32 pairs x 4
    lines = driver(ints, 5)
    assert all(line.startswith("seg ok") for line in lines)
    assert lines[1] == "seg ok passes 1" and lines[4] == "seg ok passes 2"
