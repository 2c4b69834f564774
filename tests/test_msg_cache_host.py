"""The message-cache policy (lodestar_amd/csrc/lsg_msg_cache.hpp: lookup and pin, allot, publish,
unpin, drop, clear) on the CPU, through the stand-alone driver tests/native/msgcachecheck.cpp
built with AddressSanitizer and UBSan.

A Python model of the rules -- rows FREE / PENDING / VISIBLE, pins, the CLOCK hand with one
second chance for a referenced row, epochs that void what was staged before a clear -- runs the
same scripts; every lookup result, every row assignment and every counter is compared exactly.
The caller passes the 64-bit key in, so the scripts give different messages one key.
"""
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "msgcachecheck.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]
MARK = 0x80000000  # LSG_MSG_OBJECT
HIT, PENDING, MISS = 0, 1, 2
FREE, PEND, VIS = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msgcachecheck") / "msgcachecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + FLAGS
    else:  # as tests/test_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only"] + FLAGS
    subprocess.check_call(cmd + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("msgcachecheck_cases")
    count = [0]

    def run(capacity, ops):
        """ops: list of int lists, each starting with its kind (msgcachecheck.cpp) -> output lines"""
        count[0] += 1
        ints = [capacity, len(ops)] + [x for o in ops for x in o]
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"msgcachecheck exit {p.returncode}: {p.stderr[-2000:]}"
        with open(out) as fh:
            lines = fh.read().splitlines()
        assert len(lines) == len(ops)
        return lines
    return run


class Model:
    """lsg_msg_cache.hpp restated: the same states, the same sweep, the same counters"""

    def __init__(self, capacity):
        self.resize(capacity)

    def resize(self, capacity):
        self.cap = capacity
        self.rows = [self._free() for _ in range(capacity)]
        self.hand = 0
        self.epoch = getattr(self, "epoch", 0) + 1
        self.st = dict(lookups=0, hits=0, pending=0, inserts=0, evictions=0, bypassed=0, full=0, entries=0)

    @staticmethod
    def _free():
        return dict(state=FREE, pins=0, ref=0, msg=None)

    def clear(self):
        self.rows = [self._free() for _ in range(self.cap)]
        self.hand = 0
        self.epoch += 1
        self.st["entries"] = 0

    def find(self, msg):
        for r, row in enumerate(self.rows):
            if row["state"] != FREE and row["msg"] == msg:
                return r
        return None

    def lookup(self, msg):
        self.st["lookups"] += 1
        r = self.find(msg)
        if r is None:
            return MISS, -1
        if self.rows[r]["state"] == PEND:
            self.st["pending"] += 1
            return PENDING, -1
        self.rows[r]["pins"] += 1
        self.rows[r]["ref"] = 1
        self.st["hits"] += 1
        return HIT, r

    def allot(self, msg):
        if self.find(msg) is not None:
            self.st["pending"] += 1
            return 0, -1
        for _ in range(2 * self.cap):
            r = self.hand
            self.hand = (self.hand + 1) % self.cap
            row = self.rows[r]
            if row["state"] == PEND or row["pins"]:
                continue
            if row["state"] == VIS:
                if row["ref"]:
                    row["ref"] = 0
                    continue
                self.st["evictions"] += 1
                self.st["entries"] -= 1
            self.rows[r] = dict(state=PEND, pins=0, ref=0, msg=msg)
            self.st["inserts"] += 1
            return 1, r
        self.st["full"] += 1
        return 0, -1

    def unpin(self, epoch, rows):
        if epoch != self.epoch:
            return
        for r in rows:
            if r < self.cap and self.rows[r]["pins"]:
                self.rows[r]["pins"] -= 1

    def publish(self, epoch, rows):
        if epoch != self.epoch:
            return
        for r in rows:
            if r < self.cap and self.rows[r]["state"] == PEND:
                self.rows[r]["state"] = VIS
                self.st["entries"] += 1

    def drop(self, epoch, rows):
        if epoch != self.epoch:
            return
        for r in rows:
            if r < self.cap and self.rows[r]["state"] == PEND:
                self.rows[r] = self._free()

    def stats_line(self):
        s = self.st
        return "S %d %d %d %d %d %d %d %d %d" % (s["lookups"], s["hits"], s["pending"], s["inserts"], s["evictions"],
                                                 s["bypassed"], s["full"], s["entries"], self.cap)


class Script:
    """ops for the driver and, op by op, what the model says the driver must print"""

    def __init__(self, capacity):
        self.capacity = capacity
        self.m = Model(capacity)
        self.ops, self.want = [], []

    @staticmethod
    def _msg(key, data, marked):
        return [key, len(data) | (MARK if marked else 0), len(data)] + list(data)

    def lookup(self, key, data, marked=False):
        res, row = self.m.lookup((key, bytes(data), marked))
        self.ops.append([0] + self._msg(key, data, marked))
        self.want.append(f"L {res} {row}")
        return res, row

    def allot(self, key, data, marked=False):
        ok, row = self.m.allot((key, bytes(data), marked))
        self.ops.append([1] + self._msg(key, data, marked))
        self.want.append(f"A {ok} {row}")
        return ok, row

    def _rows(self, kind, letter, fn, rows, stale):
        fn(self.m.epoch - stale, rows)
        self.ops.append([kind, stale, len(rows)] + list(rows))
        self.want.append(letter)

    def unpin(self, rows, stale=0):
        self._rows(2, "U", self.m.unpin, rows, stale)

    def publish(self, rows, stale=0):
        self._rows(3, "P", self.m.publish, rows, stale)

    def drop(self, rows, stale=0):
        self._rows(4, "D", self.m.drop, rows, stale)

    def clear(self):
        self.m.clear()
        self.ops.append([5])
        self.want.append("C")

    def stats(self):
        self.ops.append([6])
        self.want.append(self.m.stats_line())

    def bypass(self):
        self.m.st["bypassed"] += 1
        self.ops.append([7])
        self.want.append("B")

    def resize(self, capacity):
        self.m.resize(capacity)
        self.ops.append([8, capacity])
        self.want.append("R")

    def check(self, driver):
        self.stats()
        got = driver(self.capacity, self.ops)
        for k, (g, w) in enumerate(zip(got, self.want)):
            assert g == w, f"op {k} {self.ops[k][:4]}: driver {g!r}, model {w!r}"


def insert(s, key, data, marked=False):
    """one package's miss: lookup, allot, and (its launch observed complete) publish"""
    assert s.lookup(key, data, marked)[0] == MISS
    ok, row = s.allot(key, data, marked)
    if ok:
        s.publish([row])
    return ok, row


def test_equal_keys_with_different_bytes_never_hit(driver):
    s = Script(4)
    a, b, c = b"\x01" * 32, b"\x02" * 32, b"\x01" * 31 + b"\x03"
    assert insert(s, 7, a) == (1, 0)
    assert s.lookup(7, b) == (MISS, -1)       # the same key, other bytes
    assert s.lookup(7, c) == (MISS, -1)       # ... differing in the last byte only
    assert s.lookup(7, a[:31]) == (MISS, -1)  # ... a prefix
    assert insert(s, 7, b) == (1, 1)          # both live in one bucket's chain
    assert insert(s, 7 + 8, c) == (1, 2)      # (8 buckets for 4 rows: the same bucket, another key)
    for key, data, row in ((7, a, 0), (7, b, 1), (15, c, 2)):
        assert s.lookup(key, data) == (HIT, row)
        s.unpin([row])
    assert s.lookup(15, a) == (MISS, -1)      # the same bytes under another key of that bucket
    s.check(driver)


def test_marker_against_no_marker(driver):
    s = Script(4)
    data = bytes(range(64))
    assert insert(s, 9, data, marked=False) == (1, 0)
    assert s.lookup(9, data, marked=True) == (MISS, -1)
    assert insert(s, 9, data, marked=True) == (1, 1)
    assert s.lookup(9, data, marked=False) == (HIT, 0)
    assert s.lookup(9, data, marked=True) == (HIT, 1)
    assert s.m.st["entries"] == 2
    s.check(driver)


def test_lengths_0_1_192_193(driver):
    """the stager bypasses 0 and 193 bytes (MsgCache::cacheable, restated here); 1 and 192 bytes
    are stored whole and compared whole"""
    s = Script(4)
    for n in (0, 1, 192, 193):
        data = bytes((7 * k + n) & 255 for k in range(n))
        if n == 0 or n > 192:
            s.bypass()
            continue
        assert insert(s, n, data)[0] == 1
        assert s.lookup(n, data)[0] == HIT
        if n > 1:
            assert s.lookup(n, data[:-1] + bytes([data[-1] ^ 1]))[0] == MISS
    assert s.m.st["bypassed"] == 2 and s.m.st["entries"] == 2
    s.check(driver)


@pytest.mark.parametrize("capacity", [1, 4])
def test_all_rows_pinned_gives_full_and_no_insert(driver, capacity):
    s = Script(capacity)
    msgs = [bytes([k]) * 32 for k in range(capacity + 2)]
    for k in range(capacity):
        assert insert(s, k, msgs[k]) == (1, k)
    for k in range(capacity):  # a launch in flight reads every row
        assert s.lookup(k, msgs[k]) == (HIT, k)
    assert s.lookup(99, msgs[capacity]) == (MISS, -1)
    assert s.allot(99, msgs[capacity]) == (0, -1)
    assert s.m.st["full"] == 1 and s.m.st["inserts"] == capacity
    s.unpin(list(range(capacity)))
    # unpinned: referenced rows get their second chance, then the first one goes
    assert s.allot(99, msgs[capacity]) == (1, 0)
    assert s.m.st["evictions"] == 1
    s.check(driver)


@pytest.mark.parametrize("capacity", [1, 4])
def test_a_pending_entry_is_never_returned(driver, capacity):
    s = Script(capacity)
    m = b"\x55" * 48
    assert s.lookup(3, m) == (MISS, -1)
    assert s.allot(3, m) == (1, 0)
    assert s.lookup(3, m) == (PENDING, -1)   # another package, before the launch was observed
    assert s.allot(3, m) == (0, -1)          # ... and it cannot take a second row for it
    # pending rows are not evicted either: with every row pending a new message finds none
    for k in range(1, capacity):
        assert s.allot(100 + k, bytes([k]) * 8) == (1, k)
    assert s.allot(200, b"new") == (0, -1)
    assert s.m.st["full"] == 1
    s.publish([0])
    assert s.lookup(3, m) == (HIT, 0)
    assert s.m.st["lookups"] == 3 and s.m.st["pending"] == 2 and s.m.st["hits"] == 1
    s.check(driver)


def test_a_failed_package_frees_its_rows(driver):
    s = Script(4)
    a, b, c = b"a" * 32, b"b" * 32, b"c" * 32
    assert insert(s, 1, a) == (1, 0)
    assert s.lookup(1, a) == (HIT, 0)        # the failing package: one hit, two new messages
    assert s.allot(2, b) == (1, 1)
    assert s.allot(3, c) == (1, 2)
    s.unpin([0])
    s.drop([1, 2])
    assert s.lookup(2, b) == (MISS, -1) and s.lookup(3, c) == (MISS, -1)
    assert s.m.st["entries"] == 1
    # the freed rows are handed out again, and row 0 is unpinned: four more messages all fit
    for k, want in enumerate((3, 1, 2)):
        assert s.allot(10 + k, bytes([k]) * 4) == (1, want)
    s.check(driver)


def test_clock_second_chance(driver):
    """a slot's attestation data (hit again and again) outlives the singletons around it"""
    s = Script(4)
    att = b"attestation data" * 8
    assert insert(s, 1, att) == (1, 0)
    for k in range(3):
        assert insert(s, 10 + k, bytes([k]) * 32) == (1, 1 + k)
    assert s.lookup(1, att) == (HIT, 0)
    s.unpin([0])
    # the hand is at row 0: referenced, passed over once; the singleton in row 1 goes
    assert insert(s, 20, b"x" * 32) == (1, 1)
    assert s.lookup(1, att) == (HIT, 0)
    s.unpin([0])
    assert insert(s, 21, b"y" * 32) == (1, 2)
    assert insert(s, 22, b"z" * 32) == (1, 3)
    assert insert(s, 23, b"w" * 32) == (1, 1)  # row 0's bit was set again: passed over again
    # not hit since: when the hand comes round again row 0 is an ordinary victim
    assert insert(s, 24, b"v" * 32) == (1, 2)
    assert insert(s, 25, b"u" * 32) == (1, 3)
    assert insert(s, 26, b"t" * 32) == (1, 0)
    assert s.lookup(1, att) == (MISS, -1)
    assert s.m.st["evictions"] == 7
    s.check(driver)


def test_clear_while_nothing_is_pinned_and_stale_epochs(driver):
    s = Script(4)
    a, b = b"a" * 32, b"b" * 32
    assert insert(s, 1, a) == (1, 0)
    s.clear()
    assert s.lookup(1, a) == (MISS, -1) and s.m.st["entries"] == 0
    assert insert(s, 1, a) == (1, 0)
    # a launch staged before a clear: its pin and its pending row are void afterwards
    assert s.lookup(1, a) == (HIT, 0)
    assert s.allot(2, b) == (1, 1)
    s.clear()
    assert insert(s, 2, b) == (1, 0)
    assert s.lookup(2, b) == (HIT, 0)
    s.unpin([0], stale=1)      # the old launch's completion: nothing changes
    s.publish([1], stale=1)
    assert s.allot(3, b"c") == (1, 1)
    assert s.allot(4, b"d") == (1, 2)
    assert s.allot(5, b"e") == (1, 3)
    assert s.allot(6, b"f") == (0, -1)  # row 0 is still pinned by the new epoch's lookup
    s.resize(1)
    assert s.m.st["lookups"] == 0
    assert insert(s, 1, a) == (1, 0)
    s.resize(0)
    assert s.lookup(1, a) == (MISS, -1) and s.allot(1, a) == (0, -1)
    s.check(driver)


@pytest.mark.parametrize("capacity", [1, 4, 7])
def test_random_sequences_match_the_model(driver, capacity):
    """random packages -- lookups with forced key collisions, allots, then publish or drop and
    unpin, some left in flight while the next ones stage -- compared op by op"""
    rng = random.Random(1000 + capacity)
    msgs = [(rng.randrange(3), bytes(rng.randrange(256) for _ in range(rng.choice([1, 8, 32, 192]))), rng.random() < 0.3)
            for _ in range(3 * capacity + 3)]
    s = Script(capacity)
    in_flight = []
    for _ in range(400):
        pins, pend = [], []
        for key, data, marked in rng.sample(msgs, rng.randrange(1, min(len(msgs), 5))):
            res, row = s.lookup(key, data, marked)
            if res == HIT:
                pins.append(row)
            elif res == MISS:
                ok, row = s.allot(key, data, marked)
                if ok:
                    pend.append(row)
        in_flight.append((pins, pend, s.m.epoch))
        while in_flight and (len(in_flight) > 2 or rng.random() < 0.5):
            pins, pend, epoch = in_flight.pop(rng.randrange(len(in_flight)))
            stale = s.m.epoch - epoch
            s.unpin(pins, stale)
            (s.drop if rng.random() < 0.15 else s.publish)(pend, stale)
        if rng.random() < 0.02:
            s.clear()
        if rng.random() < 0.1:
            s.stats()
    st = s.m.st
    assert st["lookups"] == st["hits"] + st["pending"] + st["inserts"] + st["full"]
    assert st["hits"] and st["inserts"] and st["evictions"] and st["pending"]
    s.check(driver)


def test_two_threads_interleaving(driver):
    """two threads stage, publish and unpin over shared messages (the driver fails on a pending row
    returned by a lookup or a row allotted twice; ASan and UBSan watch the rest): the counters
    add up and nothing stays pinned or pending"""
    for capacity, n_msgs in ((1, 3), (4, 12), (8, 6)):
        line = driver(capacity, [[9, n_msgs, 20000]])[0].split()
        assert line[0] == "T"
        left, lookups, hits, pending, inserts, full, entries = (int(x) for x in line[1:])
        assert left == 0
        assert lookups == 2 * 20000 * 3 == hits + pending + inserts + full
        assert hits > 0 and inserts > 0 and entries <= capacity
