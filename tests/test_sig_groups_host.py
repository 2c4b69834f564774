"""Per-group signature sums (lsg_submit_jobs_grouped) on the CPU: the host policy in
lodestar_amd/csrc/lsg_plan.hpp -- included_sets (which sets join their group: those of jobs that
resolved to LSG_VALID) and plan_sig_groups (gather list, per-group ranges, the plan_seg chunk
plan that k_sig_agg_seg and k_seg_reduce<1> run) -- through the stand-alone driver
tests/native/groupcheck.cpp built with AddressSanitizer and UBSan.

A signature is an integer mod 2^61 - 1 and "addition" is addition mod that prime.  The driver
executes each plan as the device does (lane pairs, folds, wave butterflies, second pass); every
group's result is compared here with the direct sum over exactly its unmasked members.  Exact
comparisons only.
"""
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "groupcheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PRIME = (1 << 61) - 1
NO_GROUP = -1
# lsg_plan.hpp: a chunk is at most a wave's 32 lane pairs folding SEG_FOLD = 16 members each, so
# a group of 32 * 16 + 1 = 513 members is the shortest that needs the second pass
WAVE_PAIRS, SEG_FOLD = 32, 16
CHUNK_CAP = WAVE_PAIRS * SEG_FOLD
TWO_PASS = CHUNK_CAP + 1
LSG_VALID, LSG_INVALID, LSG_ERROR = 1, 0, 2
LSG_JOB_BATCHABLE = 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("groupcheck") / "groupcheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("groupcheck_cases")
    count = [0]

    def run(cases):
        """cases: list of int lists, each starting with its kind (groupcheck.cpp) -> output lines"""
        count[0] += 1
        ints = [len(cases)] + [x for c in cases for x in c]
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"groupcheck exit {p.returncode}: {p.stderr[-2000:]}"
        with open(out) as fh:
            lines = fh.read().splitlines()
        assert len(lines) == len(cases)
        return lines
    return run


def group_case(groups, n_groups, values, mask=None):
    ints = [0, len(groups), n_groups, 0 if mask is None else 1]
    for i, g in enumerate(groups):
        ints += [g, values[i], 1 if mask is None else mask[i]]
    return ints


def check_groups(line, groups, n_groups, values, mask=None):
    """the driver's per-group (sum, len) against the direct sums; -> (n_members, passes, ips_log2, cap, tmp)"""
    tok = line.split()
    assert tok[2 * n_groups] == "P" and len(tok) == 2 * n_groups + 6
    exp_sum, exp_len = [0] * n_groups, [0] * n_groups
    for i, g in enumerate(groups):
        if g != NO_GROUP and (mask is None or mask[i]):
            exp_sum[g] = (exp_sum[g] + values[i]) % PRIME
            exp_len[g] += 1
    got = [(int(tok[2 * g]), int(tok[2 * g + 1])) for g in range(n_groups)]
    assert got == list(zip(exp_sum, exp_len))
    return tuple(int(x) for x in tok[2 * n_groups + 1:])


def values_for(rng, n):
    return [rng.randrange(1, PRIME) for _ in range(n)]


def test_random_assignments_and_masks(driver):
    rng = random.Random(20)
    shapes = []
    for _ in range(60):
        n = rng.randrange(0, 700)
        ng = rng.choice([1, 2, 3, 7, 64, max(1, n // 3), n + 5])
        groups = [NO_GROUP if rng.random() < 0.2 else rng.randrange(ng) for _ in range(n)]
        mask = None if rng.random() < 0.4 else [rng.random() < 0.8 for _ in range(n)]
        shapes.append((groups, ng, values_for(rng, n), mask))
    lines = driver([group_case(*s) for s in shapes])
    for line, s in zip(lines, shapes):
        n_members = check_groups(line, *s)[0]
        assert n_members == sum(1 for i, g in enumerate(s[0]) if g != NO_GROUP and (s[3] is None or s[3][i]))


def test_group_lengths_around_the_wave_and_the_chunk(driver):
    """interleaved ids; lengths 0, 1, 2, 31, 32, 33 and TWO_PASS in one package: the long group
    takes two chunks and the second pass, every other group one chunk"""
    rng = random.Random(21)
    lengths = [0, 1, 2, 31, 32, 33, TWO_PASS, 0, CHUNK_CAP]
    members = [g for g, ln in enumerate(lengths) for _ in range(ln)]
    rng.shuffle(members)  # interleaved
    groups = []
    for g in members:  # a set outside every group after every third member
        groups.append(g)
        if len(groups) % 4 == 3:
            groups.append(NO_GROUP)
    vals = values_for(rng, len(groups))
    line, = driver([group_case(groups, len(lengths), vals)])
    n_members, passes, ips_log2, cap, tmp_items = check_groups(line, groups, len(lengths), vals)
    assert (n_members, passes, 1 << ips_log2, cap, tmp_items) == (sum(lengths), 2, WAVE_PAIRS, CHUNK_CAP, 2)
    # without the long group: one pass
    short = [g if g != 6 else NO_GROUP for g in groups]
    line, = driver([group_case(short, len(lengths), vals)])
    assert check_groups(line, short, len(lengths), vals)[1] == 1


@pytest.mark.parametrize("length", [1, 2, 31, 32, 33, CHUNK_CAP - 1, CHUNK_CAP, TWO_PASS, 2 * CHUNK_CAP + 1, 5000])
def test_one_group_of_each_length(driver, length):
    rng = random.Random(length)
    vals = values_for(rng, length)
    groups = [0] * length
    line, = driver([group_case(groups, 1, vals)])
    _, passes, _, cap, tmp_items = check_groups(line, groups, 1, vals)
    assert passes == (1 if length <= CHUNK_CAP else 2) and cap == min(length, CHUNK_CAP)
    assert tmp_items == (0 if length <= CHUNK_CAP else -(-length // CHUNK_CAP))


def test_empty_groups_no_groups_and_all_masked(driver):
    rng = random.Random(22)
    n = 100
    vals = values_for(rng, n)
    cases = [
        ([NO_GROUP] * n, 5, vals, None),                       # every set LSG_NO_GROUP
        ([i % 3 for i in range(n)], 3, vals, [0] * n),         # all masked
        ([i % 7 for i in range(n)], 300, vals, None),          # n_groups > set count
        ([2 * (i % 4) for i in range(n)], 8, vals, None),      # odd groups empty
        ([], 4, [], None),                                     # no sets at all
        ([0] * n, 1, vals, [i == 57 for i in range(n)]),       # one survivor
    ]
    lines = driver([group_case(*c) for c in cases])
    for line, c in zip(lines, cases):
        check_groups(line, *c)
    assert lines[0].split()[:10] == ["0"] * 10 and lines[1].split()[:6] == ["0"] * 6


def test_many_groups_take_the_work_bound_plan(driver):
    """4096 groups and more (SEG_WIDE_PAIRS / 32) fold up to SEG_FOLD_WIDE members per pair"""
    rng = random.Random(23)
    ng, n = 4100, 9000
    groups = [rng.randrange(ng) for _ in range(n)] + [7] * 700
    vals = values_for(rng, len(groups))
    mask = [rng.random() < 0.9 for _ in groups]
    lines = driver([group_case(groups, ng, vals), group_case(groups, ng, vals, mask)])
    check_groups(lines[0], groups, ng, vals)
    check_groups(lines[1], groups, ng, vals, mask)


def staging(jobs):
    """(first, count) of every job in caller order: batchable jobs are staged first"""
    first, n = [0] * len(jobs), 0
    for want in (True, False):
        for j, (cnt, flags, _st) in enumerate(jobs):
            if bool(flags & LSG_JOB_BATCHABLE) == want:
                first[j] = n
                n += cnt
    return first, n


def test_included_sets_follow_the_job_verdicts(driver):
    rng = random.Random(24)
    shapes = [
        [(1, 1, LSG_VALID)] * 5,
        [(3, 1, LSG_INVALID), (1, 1, LSG_VALID), (2, 0, LSG_VALID), (4, 0, LSG_ERROR), (0, 1, LSG_VALID)],
        [(2, 0, LSG_VALID), (3, 1, LSG_VALID), (1, 0, LSG_INVALID), (128, 1, LSG_ERROR), (5, 1, LSG_VALID)],
        [],
    ]
    for _ in range(30):
        shapes.append([(rng.choice([0, 1, 1, 2, 3, 17]), rng.choice([0, 1, 1, 3, 5]),
                        rng.choice([LSG_VALID, LSG_VALID, LSG_INVALID, LSG_ERROR])) for _ in range(rng.randrange(1, 40))])
    lines = driver([[1, len(jobs)] + [x for job in jobs for x in job] for jobs in shapes])
    for line, jobs in zip(lines, shapes):
        tok = line.split()
        first, n = staging(jobs)
        assert [int(x) for x in tok[:2 * len(jobs)]] == [x for j, job in enumerate(jobs) for x in (first[j], job[0])]
        assert tok[2 * len(jobs)] == "M"
        mask = tok[2 * len(jobs) + 1] if len(tok) > 2 * len(jobs) + 1 else ""
        exp = ["0"] * n
        for j, (cnt, _f, st) in enumerate(jobs):  # a multi-set job: all of its sets or none
            for i in range(first[j], first[j] + cnt):
                exp[i] = "1" if st == LSG_VALID else "0"
        assert mask == "".join(exp)
