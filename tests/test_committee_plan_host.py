"""Committee + bits sets (LSG_PK_BITS) on the CPU: the host policy in
lodestar_amd/csrc/lsg_plan.hpp (mode rule, bit arena, per-set plan words, lane pairs per set)
and the bit walk of lodestar_amd/csrc/lsg_bits.h that k_pk_agg_bits runs, through the
stand-alone driver tests/native/committeecheck.cpp built with AddressSanitizer and UBSan.

Committee members are small integers standing in for keys and "addition" is addition mod
2^61 - 1.  The driver stages and plans each case's sets together and executes the plan as the
kernel does (walk, distribution over lane pairs, fold, butterfly, complement); every result is
compared here with the direct sum over the participating members.  Exact comparisons only.
"""
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "committeecheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PRIME = (1 << 61) - 1
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 450, 512, 513, 2048, 2049]
WAVE_PAIRS = 32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("committeecheck") / "committeecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("committeecheck_cases")
    count = [0]

    def run(cases):
        """cases: list of cases, each a list of (members, bits: list of 0/1, raw bytes)"""
        count[0] += 1
        ints = [len(cases)]
        for sets in cases:
            ints.append(len(sets))
            for members, _bits, raw in sets:
                ints += [len(members)] + list(members) + [len(members), len(raw)] + list(raw)
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"committeecheck exit {p.returncode}: {p.stderr[-2000:]}"
        with open(out) as fh:
            lines = fh.read().splitlines()
        assert len(lines) == len(cases)
        res = []
        for line, sets in zip(lines, cases):
            tok = line.split()
            assert tok[-3] == "P" and len(tok) == 5 * len(sets) + 3
            res.append(([tuple(int(x) for x in tok[5 * i:5 * i + 5]) for i in range(len(sets))], int(tok[-2]), int(tok[-1])))
        return res
    return run


def pack(bits, garbage=None):
    """SSZ bitvector bytes of a 0/1 list (member k = bit k & 7 of byte k >> 3); garbage: an rng
    that fills the padding bits of the last byte and appends a byte of noise"""
    raw = bytearray((len(bits) + 7) // 8)
    for k, b in enumerate(bits):
        if b:
            raw[k >> 3] |= 1 << (k & 7)
    if garbage is not None:
        for k in range(len(bits), 8 * len(raw)):
            if garbage.random() < 0.7:
                raw[k >> 3] |= 1 << (k & 7)
        raw.append(garbage.randrange(256))
    return bytes(raw)


def patterns(n, rng):
    """the named bit patterns of a committee of n members"""
    out = {"none": [0] * n, "first": [1] + [0] * (n - 1), "last": [0] * (n - 1) + [1], "all": [1] * n,
           "all_but_one": [1] * n, "half": [1 if k < n // 2 else 0 for k in range(n)],
           "alternating": [k & 1 for k in range(n)]}
    out["all_but_one"][rng.randrange(n)] = 0
    rng.shuffle(out["half"])
    for name, q in (("random_1", 0.01), ("random_50", 0.5), ("random_99", 0.99)):
        out[name] = [1 if rng.random() < q else 0 for _ in range(n)]
    return out


def make_set(n, bits, rng, garbage=False):
    members = [rng.randrange(1, PRIME) for _ in range(n)]
    return members, list(bits), pack(bits, rng if garbage else None)


WIDE_PAIRS = 131072  # a launch of more lane pairs is work-bound: its fold doubles, up to 64


def check(sets, results, n_pairs, fold=4):
    """every set of one case against the direct sum, the mode rule and the layout rules"""
    used = 0
    spans = []
    for (members, bits, _raw), (got, complement, pairs, first, wanted) in zip(sets, results):
        n, p = len(bits), sum(bits)
        a = n - p
        assert got == sum(m for m, b in zip(members, bits) if b) % PRIME, (n, p)
        if p == 0:  # staged as the identity: nothing planned for it
            assert (complement, pairs, wanted) == (0, 1, 0)
        else:
            assert complement == (1 if a + 1 < p else 0), (n, p)
            assert wanted == (a if complement else p)
        assert 1 <= pairs <= WAVE_PAIRS and pairs & (pairs - 1) == 0
        assert first % pairs == 0 and first // WAVE_PAIRS == (first + pairs - 1) // WAVE_PAIRS
        # work follows the wanted count: at most `fold` members per pair until a wave's pairs are used up
        assert pairs == WAVE_PAIRS or fold * pairs >= wanted
        assert pairs == 1 or fold * (pairs // 2) < wanted
        spans.append((first, first + pairs))
        used += pairs
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two sets share a lane pair"
    assert used == n_pairs


@pytest.mark.parametrize("garbage", [False, True])
def test_every_length_and_pattern(driver, garbage):
    """one set per case and all sets of one length in one case (mixed widths in one launch)"""
    rng = random.Random(20 + garbage)
    cases = []
    for n in LENGTHS:
        sets = [make_set(n, bits, rng, garbage) for bits in patterns(n, rng).values()]
        cases.append(sets)
        cases += [[st] for st in sets]
    for sets, (results, n_pairs, fold) in zip(cases, driver(cases)):
        assert fold == 4
        check(sets, results, n_pairs)


def test_a_block_of_mixed_sets_in_one_plan(driver):
    """128 sets of differing lengths and participation planned together, widest first"""
    rng = random.Random(7)
    sets = []
    for _ in range(128):
        n = rng.choice(LENGTHS)
        q = rng.choice([0.0, 0.01, 0.5, 0.9, 0.99, 1.0])
        sets.append(make_set(n, [1 if rng.random() < q else 0 for _ in range(n)], rng, garbage=True))
    (results, n_pairs, fold), = driver([sets])
    assert fold == 4
    check(sets, results, n_pairs)


def test_a_work_bound_launch_folds_wider(driver):
    """sets that would take more than 131,072 lane pairs at 4 members per pair: the fold doubles
    until they fit (or reaches 64), and every result is still the direct sum"""
    rng = random.Random(11)
    n = 131
    base = [rng.randrange(1, PRIME) for _ in range(n)]
    bits = [k & 1 for k in range(n)]  # 65 wanted: 32 pairs at fold 4, 16 at 8
    raw = pack(bits)
    sets = [([(m + s) % PRIME for m in base], bits, raw) for s in range(4200)]
    sets[7] = make_set(450, [1] * 449 + [0], rng)  # (a narrow set among them)
    assert 32 * len(sets) > WIDE_PAIRS
    (results, n_pairs, fold), = driver([sets])
    assert fold == 8 and n_pairs <= WIDE_PAIRS
    check(sets, results, n_pairs, fold)
    assert results[0][2] == 16 and results[7][2] == 1


def test_mode_rule_at_its_boundary(driver):
    """complement exactly when a + 1 < p: a + 1 == p stays direct, a + 1 == p - 1 complements"""
    rng = random.Random(3)
    cases, want = [], []
    for p in (2, 3, 5, 17, 33, 226, 1025):
        for a, complement in ((p - 1, 0), (p - 2, 1), (p, 0), (0, 1 if p > 1 else 0)):
            bits = [1] * p + [0] * a
            rng.shuffle(bits)
            cases.append([make_set(p + a, bits, rng)])
            want.append(complement)
    for sets, (results, n_pairs, _fold), complement in zip(cases, driver(cases), want):
        check(sets, results, n_pairs)
        assert results[0][1] == complement


def test_a_set_never_gets_more_pairs_than_a_wave_holds(driver):
    """wanted counts far beyond 32 pairs x 4 members: the serial fold grows, the width does not"""
    rng = random.Random(5)
    cases = []
    for n in (259, 450, 2049, 8191):
        bits = [1 if k % 2 else 0 for k in range(n)]  # a + 1 >= p: direct, ~n / 2 wanted
        cases.append([make_set(n, bits, rng)])
    for sets, (results, n_pairs, _fold) in zip(cases, driver(cases)):
        check(sets, results, n_pairs)
        assert results[0][2] == WAVE_PAIRS and results[0][4] > 4 * WAVE_PAIRS
