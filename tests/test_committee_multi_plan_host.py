"""Sets spanning several committees (LSG_PK_BITS_MULTI) on the CPU: the host policy in
lodestar_amd/csrc/lsg_plan.hpp (shifted copy of every part into its own arena words, mode per
part, items per set, lane pairs per set, layout) and the walk across parts of
lodestar_amd/csrc/lsg_bits.h that k_pk_agg_bits_multi runs, through the stand-alone driver
tests/native/committeemulticheck.cpp built with AddressSanitizer and UBSan.

Committee members are small integers standing in for keys and "addition" is addition mod
2^61 - 1.  The driver stages and plans each case's sets together and executes the plan as the
kernel does (walk across parts with the carried skip, negated members of complement parts,
stored sums dealt round robin, butterfly); every result is compared here with the direct sum
over the participating members.  Exact comparisons only.
"""
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "committeemulticheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PRIME = (1 << 61) - 1
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 450]
PART_COUNTS = [1, 2, 3, 64]
WAVE_PAIRS = 32
WIDE_PAIRS = 131072  # a launch of more lane pairs is work-bound: its fold doubles, up to 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("committeemulticheck") / "committeemulticheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("committeemulticheck_cases")
    count = [0]

    def run(cases):
        """cases: list of (committees: list of member lists, sets: list of (ids, bits, raw))"""
        count[0] += 1
        ints = [len(cases)]
        for committees, sets in cases:
            ints.append(len(committees))
            for members in committees:
                ints += [len(members)] + list(members)
            ints.append(len(sets))
            for ids, bits, raw in sets:
                ints += [len(ids)] + list(ids) + [len(bits), len(raw)] + list(raw)
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"committeemulticheck exit {p.returncode}: {p.stderr[-2000:]}"
        with open(out) as fh:
            lines = fh.read().splitlines()
        assert len(lines) == len(cases)
        res = []
        for line, (_cm, sets) in zip(lines, cases):
            tok = line.split()
            assert tok[-3] == "P" and len(tok) == 5 * len(sets) + 3
            res.append(([tuple(int(x) for x in tok[5 * i:5 * i + 5]) for i in range(len(sets))], int(tok[-2]), int(tok[-1])))
        return res
    return run


def pack(bits, garbage=None):
    """SSZ bitvector bytes of a 0/1 list (bit k = bit k & 7 of byte k >> 3); garbage: an rng that
    fills the padding bits of the last byte and appends a byte of noise past n_pks"""
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


PATTERNS = ["empty", "full", "one_absent", "one_present", "alternating", "random_1", "random_50", "random_99"]


def pattern(name, n, rng):
    if name == "empty":
        return [0] * n
    if name == "full":
        return [1] * n
    if name == "one_absent":
        b = [1] * n
        b[rng.randrange(n)] = 0
        return b
    if name == "one_present":
        b = [0] * n
        b[rng.randrange(n)] = 1
        return b
    if name == "alternating":
        return [k & 1 for k in range(n)]
    q = {"random_1": 0.01, "random_50": 0.5, "random_99": 0.99}[name]
    return [1 if rng.random() < q else 0 for _ in range(n)]


def committees_of(lengths, rng):
    return [[rng.randrange(1, PRIME) for _ in range(n)] for n in lengths]


def make_set(committees, ids, part_bits, rng, garbage=False):
    bits = [b for pb in part_bits for b in pb]
    assert [len(pb) for pb in part_bits] == [len(committees[c]) for c in ids]
    return list(ids), bits, pack(bits, rng if garbage else None)


def part_mode(n, p):
    """(complement, wanted, items) of one part by the mode rule, computed here by hand"""
    if p == 0:
        return 0, 0, 0
    a = n - p
    complement = 1 if a + 1 < p else 0
    wanted = a if complement else p
    return complement, wanted, wanted + complement


def pairs_for(items, fold):
    pairs = 1
    while pairs < WAVE_PAIRS and fold * pairs < items:
        pairs *= 2
    return pairs


def check(committees, sets, results, n_pairs, fold=4):
    """every set of one case against the direct sum, the mode rule and the layout rules"""
    used = 0
    spans = []
    for (ids, bits, _raw), (got, pairs, first, items, ncomp) in zip(sets, results):
        want, off, want_items, want_comp = 0, 0, 0, 0
        for c in ids:
            n = len(committees[c])
            pb = bits[off:off + n]
            want += sum(m for m, b in zip(committees[c], pb) if b)
            complement, _wanted, it = part_mode(n, sum(pb))
            want_items += it
            want_comp += complement
            off += n
        assert off == len(bits)
        assert got == want % PRIME, (ids, sum(bits))
        if sum(bits) == 0:  # staged as the identity: nothing planned for it
            assert (pairs, items, ncomp) == (1, 0, 0)
        else:
            assert (items, ncomp) == (want_items, want_comp)
            assert pairs == pairs_for(items, fold)
        assert 1 <= pairs <= WAVE_PAIRS and pairs & (pairs - 1) == 0
        assert first % pairs == 0 and first // WAVE_PAIRS == (first + pairs - 1) // WAVE_PAIRS
        spans.append((first, first + pairs))
        used += pairs
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two sets share a lane pair"
    assert used == n_pairs


@pytest.mark.parametrize("k", PART_COUNTS)
@pytest.mark.parametrize("garbage", [False, True])
def test_every_length_and_pattern(driver, k, garbage):
    """lists of k parts: every length as the first part -- so that the following parts' boundaries
    fall inside bytes and words -- with every pattern on every part position in turn"""
    rng = random.Random(100 * k + garbage)
    committees = committees_of(LENGTHS, rng)
    cases = []
    for first in range(len(LENGTHS)):
        sets = []
        for pi, name in enumerate(PATTERNS):
            ids = [first] + [rng.randrange(len(LENGTHS)) for _ in range(k - 1)]
            names = [PATTERNS[(pi + e) % len(PATTERNS)] for e in range(k)]
            names[0] = name
            sets.append(make_set(committees, ids, [pattern(nm, LENGTHS[c], rng) for nm, c in zip(names, ids)], rng, garbage))
        cases.append((committees, sets))
        cases += [(committees, [st]) for st in sets[:3]]
    for (cm, sets), (results, n_pairs, fold) in zip(cases, driver(cases)):
        assert fold == 4
        check(cm, sets, results, n_pairs)


def test_one_pattern_on_every_part(driver):
    """every pattern on ALL parts of a set at once (all empty: the identity; all full: sums only)"""
    rng = random.Random(2)
    committees = committees_of(LENGTHS, rng)
    cases = []
    for k in PART_COUNTS:
        sets = []
        for name in PATTERNS:
            ids = [rng.randrange(len(LENGTHS)) for _ in range(k)]
            sets.append(make_set(committees, ids, [pattern(name, LENGTHS[c], rng) for c in ids], rng, True))
        cases.append((committees, sets))
    for (cm, sets), (results, n_pairs, _fold) in zip(cases, driver(cases)):
        check(cm, sets, results, n_pairs)


def test_hand_computed_modes_and_widths(driver):
    """the mode rule and pairs-per-set against values worked out by hand"""
    rng = random.Random(3)
    committees = committees_of([450, 450, 8, 2, 1], rng)
    ones = lambda n, p: [1] * p + [0] * (n - p)  # noqa: E731
    sets = [
        # 450 with 446 present: complement, 4 absentees + the sum = 5 items; 450 with 3 present:
        # direct, 3 items; 8 items at fold 4: 2 pairs
        make_set(committees, [0, 1], [ones(450, 446), ones(450, 3)], rng),
        # a full committee of 2: absentees 0 + 1 < 2: complement, 0 wanted, 1 item; a committee of
        # 1, present: 0 + 1 < 1 is false: direct, 1 item; 2 items: 1 pair
        make_set(committees, [3, 4], [[1, 1], [1]], rng),
        # 8 with 4 present: 4 + 1 < 4 false: direct, 4 items; with 5 present: 3 + 1 < 5:
        # complement, 3 + 1 = 4 items; 8 items: 2 pairs
        make_set(committees, [2, 2], [ones(8, 4), ones(8, 5)], rng),
        # two full committees of 450: 2 sums, 1 pair; no member taken by any pair
        make_set(committees, [0, 1], [[1] * 450, [1] * 450], rng),
        # 225 + 225 direct members = 450 items > 32 x 4: a wave's 32 pairs, the fold grows
        make_set(committees, [0, 1], [[k & 1 for k in range(450)]] * 2, rng),
        # 17 items: 8 pairs (4 x 4 = 16 < 17)
        make_set(committees, [0, 2], [ones(450, 13), ones(8, 4)], rng),
    ]
    (results, n_pairs, fold), = driver([(committees, sets)])
    assert fold == 4
    check(committees, sets, results, n_pairs)
    assert [(r[1], r[3], r[4]) for r in results] == [(2, 8, 1), (1, 2, 1), (2, 8, 1), (1, 2, 2), (32, 450, 0), (8, 17, 0)]
    # widest first: 32 pairs at 0, 8 at 32, the 2-pair sets at 40 and 42, the 1-pair sets at 44 and 45
    assert [r[2] for r in results] == [40, 44, 42, 45, 0, 32] and n_pairs == 46


def test_pairs_without_a_member_and_parts_without_one(driver):
    """33 complement parts with one absentee among them: 34 items on 16 lane pairs of which one
    takes a member (the others only sums); direct parts with no participant in between"""
    rng = random.Random(4)
    committees = committees_of([9] * 33 + [65, 7], rng)
    part_bits = [[1] * 9 for _ in range(33)]
    part_bits[20][4] = 0
    ids = list(range(33))
    sets = [make_set(committees, ids, part_bits, rng, True),
            # empty parts before, between and after parts that have members
            make_set(committees, [33, 0, 34, 1, 33], [[0] * 65, [1] * 9, [0] * 7, [0, 1] + [0] * 7, [0] * 65], rng, True)]
    (results, n_pairs, _fold), = driver([(committees, sets)])
    check(committees, sets, results, n_pairs)
    assert results[0][1:] == (16, 0, 34, 33)
    assert results[1][3:] == (2, 1)


def test_repeated_ids_in_any_order(driver):
    """a committee listed several times, descending ids: the list order defines the bit offsets"""
    rng = random.Random(5)
    committees = committees_of([33, 7, 65], rng)
    cases = []
    for ids in ([2, 2], [2, 1, 0, 1, 2], [0] * 64, [1, 0] * 32):
        for q in (0.01, 0.5, 0.99):
            sets = [make_set(committees, ids, [[1 if rng.random() < q else 0 for _ in committees[c]] for c in ids], rng, True)]
            cases.append((committees, sets))
    for (cm, sets), (results, n_pairs, _fold) in zip(cases, driver(cases)):
        check(cm, sets, results, n_pairs)


def test_an_electra_block_of_64_committee_sets(driver):
    """8 sets of 64 committees of 440-460 members at 99 %, 90 % and 50 %: far more than 32 x fold
    items at 50 %, a few hundred at 99 %, planned together with narrow sets"""
    rng = random.Random(6)
    lengths = [rng.randrange(440, 461) for _ in range(64)]
    committees = committees_of(lengths + [1, 2], rng)
    sets = []
    for q in (0.99, 0.99, 0.9, 0.9, 0.5, 0.5, 1.0, 0.0):
        ids = list(range(64))
        rng.shuffle(ids)
        sets.append(make_set(committees, ids, [[1 if rng.random() < q else 0 for _ in committees[c]] for c in ids], rng, True))
    sets.append(make_set(committees, [64], [[1]], rng))
    sets.append(make_set(committees, [65, 64], [[0, 1], [0]], rng))
    (results, n_pairs, fold), = driver([(committees, sets)])
    assert fold == 4
    check(committees, sets, results, n_pairs)
    assert results[4][1] == WAVE_PAIRS and results[4][3] > 64 * WAVE_PAIRS
    assert results[6][1:] == (16, 32 * 6, 64, 64)  # all present: 64 sums


def test_a_work_bound_launch_folds_wider(driver):
    """sets that would take more than 131,072 lane pairs at 4 items per pair: the fold doubles
    until they fit, and every result is still the direct sum"""
    rng = random.Random(11)
    committees = committees_of([65, 66], rng)
    bits = [[k & 1 for k in range(65)], [k & 1 for k in range(66)]]  # 32 + 33 = 65 items: 32 pairs at 4, 16 at 8
    one = make_set(committees, [0, 1], bits, rng)
    sets = [one] * 4200
    sets[7] = make_set(committees, [1, 0], [[1] * 66, [1] * 64 + [0]], rng)  # (a narrow set among them)
    assert 32 * len(sets) > WIDE_PAIRS
    (results, n_pairs, fold), = driver([(committees, sets)])
    assert fold == 8 and n_pairs <= WIDE_PAIRS
    check(committees, sets, results, n_pairs, fold)
    assert results[0][1] == 16 and results[7][1] == 1
