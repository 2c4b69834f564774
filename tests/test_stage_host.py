"""Package staging on the CPU: lodestar_amd/csrc/lsg_stage.hpp (the staging arena's layout, the
distinct-message table and its sample rule, the message-cache decisions, committee and key-slot
staging, the RLC randomizers) and the two lists of lodestar_amd/csrc/lsg_plan.hpp that a package
appends next (KeyValidate, per-message sets), through the stand-alone driver
tests/native/stagecheck.cpp, built once with AddressSanitizer and UBSan and once plainly and run
directly.

The driver allocates the arena at exactly StageLayout::bytes, the bit arena at exactly the
measured words and every caller buffer at exactly its stated length, and fills both arenas with
0xa5 first.  A model written here independently -- message ids by first occurrence over (length
word, bytes), the key-slot rule, the bit fields, splitmix64 with zeros skipped, the message
cache's rules (the model of tests/test_msg_cache_host.py) called in the expected order --
predicts every result field, every arena byte (untouched ones included), the plan words and the
bit words.  Exact comparisons only; a failed compile is an error.
"""
import os
import random
import shutil
import subprocess

import pytest

from tests.test_msg_cache_host import HIT, MISS, Model as CacheModel

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "stagecheck.cpp")
BUILDS = {"plain": ["-O2"],
          "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
MARK = 0x80000000    # LSG_MSG_OBJECT
MC_ROW = 0x80000000  # a source word that names a cache row
PK_INDEX, PK_BITS, PK_MULTI = 4, 8, 12
BAD_COMMITTEE, ERR_ENTROPY = 103, 7
FILL = 0xa5
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the script's objects
class Set:
    def __init__(self, msg=b"m", msg_len=None, sig=b"", sig_len=None, pks=None, pk_len=48, n_pks=0, noscale=2, rnd_in=0,
                 key=None):
        self.msg = msg  # None: a null pointer
        self.msg_len = (len(msg) if msg is not None else 0) if msg_len is None else msg_len
        self.sig = sig
        self.sig_len = (len(sig) if sig is not None else 0) if sig_len is None else sig_len
        self.pks, self.pk_len, self.n_pks = pks, pk_len, n_pks
        self.noscale, self.rnd_in, self.key = noscale, rnd_in, key

    def ints(self):
        out = []
        for ln, b in ((self.sig_len, self.sig), (self.msg_len, self.msg)):
            out += [ln, 0 if b is None else 1, 0 if b is None else len(b)] + list(b or b"")
        out += [self.n_pks, self.pk_len, 0 if self.pks is None else 1, 0 if self.pks is None else len(self.pks)]
        out += list(self.pks or b"") + [self.noscale, self.rnd_in, self.key or 0]
        return out


_r = random.Random(77)


def rbytes(n):
    return bytes(_r.randrange(256) for _ in range(n))


def keys_set(msg, n_keys=1, pk_len=48, **kw):
    return Set(msg=msg, sig=rbytes(96), pks=rbytes(pk_len * n_keys), pk_len=pk_len, n_pks=n_keys, **kw)


def index_set(msg, indices, **kw):
    return Set(msg=msg, sig=rbytes(96), pks=b"".join(i.to_bytes(4, "little") for i in indices), pk_len=PK_INDEX,
               n_pks=len(indices), **kw)


def pack(bits, garbage=True):
    """SSZ bitvector bytes; garbage: noise in the padding bits of the last byte"""
    raw = bytearray((len(bits) + 7) // 8)
    for k, b in enumerate(bits):
        raw[k >> 3] |= b << (k & 7)
    for k in range(len(bits), 8 * len(raw)):
        if garbage and _r.random() < 0.7:
            raw[k >> 3] |= 1 << (k & 7)
    return bytes(raw)


def bits_set(msg, cid, bits, **kw):
    return Set(msg=msg, sig=rbytes(96), pks=cid.to_bytes(4, "little") + pack(bits), pk_len=PK_BITS, n_pks=len(bits), **kw)


def multi_set(msg, ids, bits, count=None, n_pks=None, **kw):
    blob = (len(ids) if count is None else count).to_bytes(4, "little") + b"".join(i.to_bytes(4, "little") for i in ids)
    return Set(msg=msg, sig=rbytes(96), pks=blob + pack(bits), pk_len=PK_MULTI, n_pks=len(bits) if n_pks is None else n_pks,
               **kw)


class Case:
    def __init__(self, sets, committees=(), cache=None, cache_ops=(), scale=False, dedup=False, dedup_on=True,
                 bits_ok=True, seed=0, keymode=False, plan_prefix=0, entropy=(), jobs=(), lists=None):
        self.sets, self.committees = list(sets), list(committees)  # committees: (ok, len) per id
        self.cache, self.cache_ops = cache, list(cache_ops)        # cache: capacity or None (no cache given)
        self.scale, self.dedup, self.dedup_on, self.bits_ok = scale, dedup, dedup_on, bits_ok
        self.seed, self.keymode, self.plan_prefix = seed, keymode, plan_prefix
        self.entropy = list(entropy)  # (ok, words) per call
        self.jobs = list(jobs)        # (flags, n_sets) per job
        self.lists = lists            # (first, len): plan_msg_lists over that group

    def key_of(self, s):
        return s.key if self.keymode else msg_key(s.msg or b"", s.msg_len)

    def ints(self):
        out = [0, len(self.committees)] + [x for c in self.committees for x in c]
        out += [0 if self.cache is None else 1, self.cache or 0, len(self.cache_ops)]
        for op in self.cache_ops:
            if op[0] in ("lookup", "allot"):
                _, key, msg, marked = op
                out += [0 if op[0] == "lookup" else 1, key, len(msg) | (MARK if marked else 0), len(msg)] + list(msg)
            else:
                out += [2 if op[0] == "unpin" else 3, len(op[1])] + list(op[1])
        out += [int(self.scale), int(self.dedup), int(self.dedup_on), int(self.bits_ok), self.seed, int(self.keymode),
                self.plan_prefix, len(self.entropy)]
        for ok, words in self.entropy:
            out += [int(ok), len(words)] + list(words)
        out += [len(self.jobs)] + [x for j in self.jobs for x in j]
        out += [1, self.lists[0], self.lists[1]] if self.lists else [0, 0, 0]
        out += [len(self.sets)] + [x for s in self.sets for x in s.ints()]
        return out


# ---------------------------------------------------------------- the model
def msg_key(m, len_word):
    h = 0x9e3779b97f4a7c15 ^ len_word
    n, k = len_word & ~MARK, 0
    while k + 8 <= n:
        h = ((h ^ int.from_bytes(m[k:k + 8], "little")) * 0xff51afd7ed558ccd) & M64
        h ^= h >> 32
        k += 8
    while k < n:
        h = ((h ^ m[k]) * 0x100000001b3) & M64
        k += 1
    return h ^ (h >> 29)


def splitmix(seed):
    s = seed
    while True:
        s = (s + 0x9e3779b97f4a7c15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        yield z ^ (z >> 31)


def layout(n, npk, stride, mb):
    """offsets by the stated rule: the nine fields in order, each on the next multiple of 8"""
    nn, np_, mb = max(n, 1), max(npk, 1), max(mb, 1)
    sizes = [("sig", 192 * nn), ("siglen", 4 * nn), ("msgoff", 4 * nn), ("msglen", 4 * nn), ("mid", 4 * nn),
             ("pklen", 4 * np_), ("rnd", 8 * nn), ("pk", stride * np_), ("msg", mb)]
    L, at = {}, 0
    for name, size in sizes:
        at = (at + 7) // 8 * 8
        L[name] = at
        at += size
    L["bytes"] = at
    return L, dict(sizes)


def staging_order(case):
    """indices of case.sets in staging order: batchable jobs first, each kind in caller order"""
    if not case.jobs:
        return list(range(len(case.sets))), []
    first, spans = 0, []
    for flags, cnt in case.jobs:
        spans.append((flags, list(range(first, first + cnt))))
        first += cnt
    order, jobs = [], []
    for want in (1, 0):
        for j, (flags, idx) in enumerate(spans):
            if (flags & 1) == want:
                jobs.append((j, flags, len(order), len(idx)))
                order += idx
    return order, sorted(jobs)


def popcount(bits):
    return sum(bits)


def field_bits(raw, off, n):
    return [(raw[(off + k) >> 3] >> ((off + k) & 7)) & 1 for k in range(n)]


def words_of_bits(bits):
    w = [0] * ((len(bits) + 31) // 32)
    for k, b in enumerate(bits):
        w[k >> 5] |= b << (k & 31)
    return w


def model(case):
    order, jobs = staging_order(case)
    sets = [case.sets[i] for i in order]
    n = len(sets)
    bits_kind = lambda s: case.bits_ok and s.pk_len == PK_BITS  # noqa: E731
    multi_kind = lambda s: case.bits_ok and s.pk_len == PK_MULTI  # noqa: E731
    plain = [s for s in sets if not bits_kind(s) and not multi_kind(s)]
    npk = sum(s.n_pks for s in plain)
    all_index = all(s.pk_len == PK_INDEX for s in plain if s.n_pks)
    msg_total = sum(s.msg_len & ~MARK for s in sets)
    n_bits, n_multi = sum(map(bits_kind, sets)), sum(map(multi_kind, sets))
    bit_words = 0
    for s in sets:
        if bits_kind(s):
            bit_words += (s.n_pks + 31) // 32
        elif multi_kind(s):
            k = int.from_bytes(s.pks[:4], "little") if s.pks is not None else None
            bit_words += (s.n_pks + 31) // 32 + (k if k is not None and k <= 64 else 0)
    exp = {"sizes": [npk, msg_total, n_bits, n_multi, bit_words, int(all_index), int(any(s.msg_len & MARK for s in sets))]}
    stride = 4 if all_index else 96
    L, size = layout(n, npk, stride, msg_total)
    exp["layout"] = [L[k] for k in ("sig", "siglen", "msgoff", "msglen", "mid", "pklen", "rnd", "pk", "msg", "bytes")]
    A = bytearray([FILL]) * L["bytes"]
    cbits = [int.from_bytes(bytes([FILL]) * 4, "little")] * bit_words

    def w32(field, i, v):
        A[L[field] + 4 * i:L[field] + 4 * i + 4] = (v & 0xffffffff).to_bytes(4, "little")

    for f in ("siglen", "msgoff", "msglen", "pklen"):
        w32(f, 0, 0)
    A[L["rnd"]:L["rnd"] + 8] = bytes(8)
    # the message cache as primed by the script
    cache = CacheModel(case.cache or 0)
    for op in case.cache_ops:
        if op[0] == "lookup":
            cache.lookup((op[1], bytes(op[2]), op[3]))
        elif op[0] == "allot":
            cache.allot((op[1], bytes(op[2]), op[3]))
        elif op[0] == "unpin":
            cache.unpin(cache.epoch, op[1])
        else:
            cache.publish(cache.epoch, op[1])
    dedup = case.dedup and case.dedup_on
    mc = cache if dedup and case.cache else None
    keys = [case.key_of(s) for s in sets]
    table = False
    if dedup and n > 0:
        k = min(n, 256)
        sample = [keys[j * (n // k)] for j in range(k)]
        table = mc is not None or (n > 1 and len(set(sample)) < len(sample))
    plan = [7] * case.plan_prefix
    src_off = len(plan)
    seen, ids = {}, []
    mo = po = bw = nm = n_miss = hits = 0
    pins, pend, store, src = [], [], [], []
    miss_obj = False
    pk_cnt, pk_first = [], []
    bits_p, bits_kerr = [-1] * n, [0] * n
    bset, mset, mparts = [], [], []
    registered = lambda c: c < len(case.committees) and case.committees[c][0]  # noqa: E731
    for i, s in enumerate(sets):
        w32("siglen", i, s.sig_len)
        at = L["sig"] + 192 * i
        if s.sig_len in (96, 192) and s.sig is not None:
            A[at:at + s.sig_len] = s.sig[:s.sig_len]
        else:
            A[at:at + 96] = bytes(96)
        mb = s.msg_len & ~MARK
        ident = (s.msg_len, bytes((s.msg or b"")[:mb]), keys[i]) if table else ("set", i)
        new = ident not in seen
        if new:
            seen[ident] = nm
        ids.append(seen[ident])
        w32("mid", i, seen[ident])
        if new:
            slot = nm
            staged = True
            if mc is not None:
                row, hit, st = -1, False, False
                if not (0 < mb <= 192) or s.msg is None:
                    cache.st["bypassed"] += 1
                else:
                    who = (keys[i], bytes(s.msg[:mb]), bool(s.msg_len & MARK))
                    res, row = cache.lookup(who)
                    hit = res == HIT
                    if res == MISS:
                        st, row = cache.allot(who)
                if hit:
                    pins.append(row)
                    hits += 1
                    src.append(MC_ROW | row)
                    staged = False
                else:
                    slot = n_miss
                    n_miss += 1
                    if st:
                        pend.append(row)
                        store += [slot, row]
                    src.append(slot)
                    miss_obj = miss_obj or bool(s.msg_len & MARK)
            if staged:
                w32("msgoff", slot, mo)
                w32("msglen", slot, s.msg_len)
                A[L["msg"] + mo:L["msg"] + mo + mb] = (s.msg or b"")[:mb]
                mo += mb
            nm += 1
        pk_first.append(po)
        if bits_kind(s):
            pk_cnt.append(0)
            cid = int.from_bytes(s.pks[:4], "little") if s.pks is not None else None
            rec = (0, 0, 0, 0, i)
            if cid is None or not registered(cid) or case.committees[cid][1] != s.n_pks:
                bits_kerr[i] = BAD_COMMITTEE
            else:
                field = field_bits(s.pks[4:], 0, s.n_pks)
                if popcount(field):
                    rec = (cid, bw, s.n_pks, popcount(field), i)
                    nw, nb = (s.n_pks + 31) // 32, (s.n_pks + 7) // 8
                    raw = s.pks[4:4 + nb] + bytes(4 * nw - nb)  # the caller's bytes as they are, padding included
                    cbits[bw:bw + nw] = [int.from_bytes(raw[4 * k:4 * k + 4], "little") for k in range(nw)]
                    bw += nw
            bits_p[i] = rec[3]
            bset += rec
            continue
        if multi_kind(s):
            pk_cnt.append(0)
            rec = (len(mparts) // 4, 0, 0, 0, i)
            k = int.from_bytes(s.pks[:4], "little") if s.pks is not None else None
            ok = k is not None and k <= 64 and (k > 0 or s.n_pks == 0)
            cids = [int.from_bytes(s.pks[4 + 4 * e:8 + 4 * e], "little") for e in range(k)] if ok else []
            ok = ok and all(registered(c) for c in cids)
            if not ok or sum(case.committees[c][1] for c in cids) != s.n_pks:
                bits_kerr[i] = BAD_COMMITTEE
            else:
                raw = s.pks[4 + 4 * k:]
                if popcount(field_bits(raw, 0, s.n_pks)):
                    off = n_parts = p_all = items = 0
                    for c in cids:
                        ln = case.committees[c][1]
                        part = field_bits(raw, off, ln)
                        off += ln
                        p = popcount(part)
                        if not p:
                            continue
                        mparts += [c, bw, ln, p]
                        w = words_of_bits(part)
                        cbits[bw:bw + len(w)] = w
                        bw += len(w)
                        n_parts += 1
                        p_all += p
                        complement = (ln - p) + 1 < p
                        items += (ln - p) + 1 if complement else p
                    rec = (rec[0], n_parts, p_all, items, i)
            bits_p[i] = rec[2]
            mset += rec
            continue
        pk_cnt.append(s.n_pks)
        for q in range(s.n_pks):
            if all_index:
                w32("pklen", po, PK_INDEX)
                A[L["pk"] + 4 * po:L["pk"] + 4 * po + 4] = s.pks[4 * q:4 * q + 4] if s.pks is not None else bytes(4)
            else:
                w32("pklen", po, s.pk_len)
                at = L["pk"] + 96 * po
                if s.pk_len in (48, 96, PK_INDEX) and s.pks is not None:
                    A[at:at + s.pk_len] = s.pks[s.pk_len * q:s.pk_len * (q + 1)]
                else:
                    A[at:at + 4] = bytes(4)
            po += 1
    assert po == npk and bw <= bit_words and len(A) == L["bytes"]
    if mc is not None:
        plan += src + store
    by_bits = n_bits + n_multi
    exp["res"] = [n, npk, stride, nm, int(nm < n), int(miss_obj if mc is not None else bool(exp["sizes"][6])),
                  int(n > 0 and by_bits == 0 and all(s.n_pks == 1 for s in sets)), int(n > 0 and by_bits == n),
                  int(mc is not None), n_miss, hits, src_off if mc is not None else None,
                  src_off + nm if mc is not None else None, mo, bw, cache.epoch if mc is not None else None]
    # the randomizers
    rc, calls, rnd = 0, 0, [0] * n
    if n and case.scale:
        if sets[0].rnd_in:
            rnd = [s.rnd_in for s in sets]
        elif case.seed:
            g = splitmix(case.seed)
            rnd = [next(x for x in g if x) for _ in range(n)]
        else:
            script = iter(case.entropy)
            ok, words = next(script)
            calls = 1
            if not ok:
                rc = ERR_ENTROPY
            else:
                rnd = list(words)
                for i in range(n):
                    while rc == 0 and rnd[i] == 0:
                        ok, words = next(script)
                        calls += 1
                        if ok:
                            rnd[i] = words[0]
                        else:
                            rc = ERR_ENTROPY
        if rc == 0 and any(s.noscale != 2 for s in sets):
            rnd = [0 if s.noscale == 1 else r for s, r in zip(sets, rnd)]
    if n:  # (what a failed draw leaves in the arena is whatever the source had written: not compared)
        A[L["rnd"]:L["rnd"] + 8 * n] = b"".join(r.to_bytes(8, "little") for r in rnd)
    exp["rc"], exp["entropy_calls"] = [rc], [calls]
    if rc == 0:
        exp["rnd"] = rnd
    if nm < n:
        exp["msg_id"] = ids
    exp.update(pins=pins, pend=pend, store=store, pk_cnt=pk_cnt, pk_first=pk_first, bits_sets=bset, multi_sets=mset,
               multi_parts=mparts, bits_p=bits_p if by_bits else [], bits_kerr=bits_kerr if by_bits else [])
    for f in ("siglen", "msgoff", "msglen", "mid", "pklen"):
        exp["a_" + f] = [int.from_bytes(A[L[f] + 4 * k:L[f] + 4 * k + 4], "little") for k in range(size[f] // 4)]
    if rc == 0:
        exp["a_rnd"] = [int.from_bytes(A[L["rnd"] + 8 * k:L["rnd"] + 8 * k + 8], "little") for k in range(max(n, 1))]
    for f in ("sig", "pk", "msg"):
        exp["a_" + f] = bytes(A[L[f]:L[f] + size[f]]).hex()
    exp["cbits"] = cbits
    st = cache.st
    exp["mcstats"] = [st[k] for k in ("lookups", "hits", "pending", "inserts", "evictions", "bypassed", "full", "entries")]
    # the KeyValidate list: the byte keys of flagged jobs, in staging order, then the set of each
    if jobs and rc == 0:
        listed = [0] * n
        for _j, flags, first, cnt in jobs:
            for i in range(first, first + cnt):
                if flags & 4 and sets[i].pk_len not in (PK_INDEX, PK_BITS, PK_MULTI) and pk_cnt[i]:
                    listed[i] = 1
        kv = [(pk_first[i] + q, i) for i in range(n) if listed[i] for q in range(pk_cnt[i])]
        exp["kv"] = [len(kv), len(plan) if kv else 0]
        exp["kv_set"] = listed if kv else []
        plan += [a for a, _ in kv] + [b for _, b in kv]
    # the per-message lists of sets [first, first + len): each message's sets in order, then one
    # chunk (offset, length, destination) per message -- every list here is far below one lane
    # pair's 16 serial folds, so one pass of one-pair chunks reduces them
    if case.lists and rc == 0:
        first, ln = case.lists
        per = [[i for i in range(first, first + ln) if ids[i] == m] for m in range(nm)]
        assert max(map(len, per)) <= 16 and ln / nm < 8
        idx_off = len(plan)
        plan += [i for lst in per for i in lst]
        exp["msum"] = [0, 1, idx_off, 0, 1, 0, nm, len(plan), 0, 1]
        at = 0
        for m, lst in enumerate(per):
            plan += [at, len(lst), m]
            at += len(lst)
    exp["plan"] = plan
    return exp


# ---------------------------------------------------------------- the driver
@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stagecheck_" + request.param) / "stagecheck")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-std=c++17"]
    else:  # as tests/test_committee_multi_plan_host.py: the build's own compiler, host side only
        from lodestar_amd.build import hipcc
        cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17"]
    subprocess.check_call(cmd + BUILDS[request.param] + [SRC, "-o", exe])
    work = tmp_path_factory.mktemp("stagecheck_cases_" + request.param)
    count = [0]

    def run(items):
        """items: Case objects or ("layout", n, npk, stride, mb) -> per item {line name: tokens}"""
        count[0] += 1
        ints = [len(items)]
        for it in items:
            ints += it.ints() if isinstance(it, Case) else [1] + list(it[1:])
        src, out = str(work / f"c{count[0]}.txt"), str(work / f"o{count[0]}.txt")
        with open(src, "w") as fh:
            fh.write(" ".join(str(int(x)) for x in ints))
        p = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, f"stagecheck exit {p.returncode}: {p.stderr[-3000:]}"
        res, cur = [], {}
        with open(out) as fh:
            for line in fh.read().splitlines():
                tok = line.split()
                if tok[0] == "end":
                    res.append(cur)
                    cur = {}
                else:
                    cur[tok[0]] = tok[1:]
        assert len(res) == len(items) and not cur
        return res
    return run


def check(driver, cases):
    """every case of one script (one Staged and one table serve them all, in order) against the model"""
    for k, (case, got) in enumerate(zip(cases, driver(cases))):
        exp = model(case)
        for name, want in exp.items():
            have = got[name]
            if isinstance(want, str):
                assert have == ([want] if want else []), (k, name)
            else:
                assert len(have) == len(want), (k, name, have, want)
                mask = 0xffffffff if name == "plan" else -1  # (plan words are printed as int32)
                for j, (h, w) in enumerate(zip(have, want)):
                    assert w is None or int(h) & mask == w, (k, name, j, h, w)
        # (lines the model leaves out are those a failed draw or a package without repeats leaves stale)
        assert set(got) - set(exp) <= {"rnd", "a_rnd", "msg_id"}, (k, set(got) - set(exp))
    return [model(c) for c in cases]


def msgs(k):
    return [b"message-%03d-" % i + bytes([i & 255]) * 19 for i in range(k)]  # 32 bytes each


# ---------------------------------------------------------------- sets, keys, signatures
def test_empty_and_single_packages(driver):
    m = msgs(2)
    check(driver, [Case([]), Case([], scale=True, seed=5, dedup=True), Case([keys_set(m[0])]),
                   Case([keys_set(m[0])], scale=True, seed=5, dedup=True, bits_ok=False), Case([])])


def test_key_slots(driver):
    m = msgs(8)
    exp = check(driver, [
        # all indices: 4-byte slots; a set without a key blob stages zeros
        Case([index_set(m[0], [5]), index_set(m[1], [1, 2, 3]), Set(msg=m[2], pks=None, pk_len=PK_INDEX, n_pks=2),
              index_set(m[3], [])]),
        # one 48-byte key among indices: 96-byte slots for all
        Case([index_set(m[0], [5, 6]), keys_set(m[1], 1), index_set(m[2], [9])]),
        # unknown lengths (8 is one where bits are not accepted) and a null blob: the slot's first
        # word zeroed, the length kept for the decoder to refuse
        Case([keys_set(m[0], 2, pk_len=96), Set(msg=m[1], pks=rbytes(24), pk_len=12, n_pks=2),
              Set(msg=m[2], pks=b"", pk_len=0, n_pks=1), Set(msg=m[3], pks=rbytes(16), pk_len=PK_BITS, n_pks=2),
              Set(msg=m[4], pks=None, pk_len=48, n_pks=1), keys_set(m[5], 0)], bits_ok=False),
        # one key each: single_keys; one two-key set: not
        Case([keys_set(x) for x in m[:4]]),
        Case([keys_set(m[0]), keys_set(m[1], 2), keys_set(m[2])]),
        Case([index_set(x, [3]) for x in m[:3]]),
    ])
    assert [e["res"][2] for e in exp] == [4, 96, 96, 96, 96, 4]
    assert [e["res"][6] for e in exp] == [0, 0, 0, 1, 0, 1]


def test_signatures(driver):
    m = msgs(6)
    check(driver, [Case([Set(msg=m[0], sig=rbytes(96)), Set(msg=m[1], sig=rbytes(192)), Set(msg=m[2], sig=b""),
                         Set(msg=m[3], sig=rbytes(95)), Set(msg=m[4], sig=None, sig_len=96),
                         Set(msg=m[5], sig=None, sig_len=0)])])


# ---------------------------------------------------------------- messages
def test_messages_repeats_markers_and_equal_keys(driver):
    a, b = rbytes(160), rbytes(160)
    m = msgs(4)
    sets = [keys_set(m[0]), keys_set(b""), keys_set(m[1]), keys_set(m[0]), keys_set(None), keys_set(a),
            keys_set(a, msg_len=160 | MARK), keys_set(m[1]), keys_set(b""), keys_set(a), keys_set(rbytes(13)),
            keys_set(a, msg_len=160 | MARK)]
    exp = check(driver, [Case(sets, dedup=True), Case(sets, dedup=True, dedup_on=False), Case(sets, dedup=False),
                         Case(sets[:5], dedup=True)])
    # the empty message and the null one are one message; marked and unmarked bytes are two
    assert exp[0]["msg_id"] == [0, 1, 2, 0, 1, 3, 4, 2, 1, 3, 5, 4] and exp[0]["res"][3:6] == [6, 1, 1]
    assert exp[1]["res"][3:5] == [12, 0] and exp[2]["res"][3:5] == [12, 0]
    # two different messages forced onto one key stay distinct, equal ones are still found
    forced = [keys_set(m[0], key=9), keys_set(m[1], key=9), keys_set(m[2], key=9), keys_set(m[1], key=9),
              keys_set(m[3], key=1 << 63), keys_set(m[0], key=9)]
    exp = check(driver, [Case(forced, dedup=True, keymode=True)])
    assert exp[0]["msg_id"] == [0, 1, 2, 1, 3, 0]


def test_the_sample_rule(driver):
    """300 sets whose only repeat the 256-set sample (sets 0..255) does not visit: staged without the
    table, every set its own message; with a cache given the table is always built"""
    m = msgs(300)
    sets = [Set(msg=x, sig=None, sig_len=0, pks=None, pk_len=PK_INDEX, n_pks=1) for x in m]
    sets[299] = Set(msg=m[270], sig=None, sig_len=0, pks=None, pk_len=PK_INDEX, n_pks=1)
    seen = list(sets)
    seen[100] = Set(msg=m[3], sig=None, sig_len=0, pks=None, pk_len=PK_INDEX, n_pks=1)
    exp = check(driver, [Case(sets, dedup=True), Case(sets, dedup=True, cache=512), Case(sets, dedup=False, cache=512),
                         Case(seen, dedup=True)])
    assert exp[0]["res"][3:5] == [300, 0] and exp[0]["res"][8] == 0
    assert exp[1]["res"][3:5] == [299, 1] and exp[1]["msg_id"][299] == 270 and exp[1]["res"][8:11] == [1, 299, 0]
    assert exp[2]["res"][3:5] == [300, 0] and exp[2]["res"][8] == 0 and exp[2]["mcstats"] == [0] * 8
    assert exp[3]["res"][3:5] == [298, 1]


def test_messages_that_differ_only_in_length(driver):
    """m, m || 0x00, m || 0x00 0x00, m[:-1] and the empty message are five messages to the table and
    to the cache (a hit on m and on m || 0x00 leaves the other two siblings misses); staged back
    to back at 33, 34, 35 and 32 bytes, every later message starts at an odd offset; the cache
    takes 191 and 192 bytes and lets 193 pass"""
    m, long_msg = rbytes(33), rbytes(193)
    sib = [m, m + b"\0", m + b"\0\0", m[:-1], b""]
    sets = [keys_set(sib[i % 5]) for i in range(20)]
    edge = [keys_set(long_msg[:191]), keys_set(long_msg[:192]), keys_set(long_msg), keys_set(long_msg[:192] + b"\xff"),
            keys_set(long_msg[:191])]
    k = lambda x: msg_key(x, len(x))  # noqa: E731
    primed = [("lookup", k(sib[0]), sib[0], False), ("allot", k(sib[0]), sib[0], False), ("publish", [0]),
              ("lookup", k(sib[1]), sib[1], False), ("allot", k(sib[1]), sib[1], False), ("publish", [1])]
    exp = check(driver, [Case(sets, dedup=True), Case(sets, dedup=False), Case(sets + edge, dedup=True, cache=16),
                         Case(sets + edge, dedup=True, cache=16, cache_ops=primed)])
    assert exp[0]["msg_id"] == [i % 5 for i in range(20)] and exp[0]["res"][3:5] == [5, 1]
    assert exp[1]["res"][3:5] == [20, 0]
    # the 191-byte message repeats; lookups: the four siblings with bytes, 191 and 192; the empty
    # message and the two of 193 bytes bypass
    assert exp[2]["msg_id"][20:] == [5, 6, 7, 8, 5] and exp[2]["res"][3] == 9 and exp[2]["res"][8:11] == [1, 9, 0]
    assert exp[2]["mcstats"][:6] == [6, 0, 0, 6, 0, 3]
    assert exp[3]["res"][8:11] == [1, 7, 2] and exp[3]["pins"] == [0, 1]
    assert exp[3]["mcstats"][:6] == [8, 2, 0, 6, 0, 3]


# ---------------------------------------------------------------- the message cache
def test_cache_hit_miss_pending_full_and_bypass(driver):
    m = msgs(8)
    long_msg, marked = rbytes(193), rbytes(160)
    k = lambda x, w=None: msg_key(x, len(x) if w is None else w)  # noqa: E731
    visible = [("lookup", k(m[0]), m[0], False), ("allot", k(m[0]), m[0], False), ("publish", [0]),
               ("lookup", k(marked, 160 | MARK), marked, True), ("allot", k(marked, 160 | MARK), marked, True),
               ("publish", [1]), ("lookup", k(m[1]), m[1], False), ("allot", k(m[1]), m[1], False)]  # (row 2: pending)
    sets = [keys_set(m[2]), keys_set(m[0]), keys_set(m[1]), keys_set(long_msg), keys_set(m[2]),
            keys_set(marked, msg_len=160 | MARK), keys_set(marked), keys_set(b""), keys_set(m[0]), keys_set(m[3]),
            keys_set(None)]
    exp = check(driver, [
        Case(sets, dedup=True, cache=8, cache_ops=visible, plan_prefix=3),
        # a full cache: both rows pending, so no miss is stored
        Case([keys_set(m[4]), keys_set(m[5]), keys_set(m[4])], dedup=True, cache=2,
             cache_ops=[("allot", 1, b"x", False), ("allot", 2, b"y", False)]),
        # a marked message among the misses only: msg_objs follows the misses
        Case([keys_set(marked, msg_len=160 | MARK), keys_set(m[6])], dedup=True, cache=8, cache_ops=visible),
        Case([keys_set(rbytes(160), msg_len=160 | MARK), keys_set(m[0])], dedup=True, cache=8, cache_ops=visible),
        # the switch off, or no dedup asked: the cache is left alone
        Case(sets, dedup=True, dedup_on=False, cache=8, cache_ops=visible),
        # injected keys: a different message on a cached message's key misses
        Case([keys_set(m[1], key=k(m[0])), keys_set(m[0], key=k(m[0]))], dedup=True, cache=8, cache_ops=visible[:3],
             keymode=True),
    ])
    e = exp[0]
    # distinct: m2, m0 (hit row 0), m1 (pending), long (bypass), marked (hit row 1), unmarked bytes, empty (bypass), m3
    assert e["res"][3] == 8 and e["res"][8:13] == [1, 6, 2, 3, 11]
    assert e["pins"] == [0, 1] and e["pend"] == [3, 4, 5] and e["store"] == [0, 3, 3, 4, 5, 5]
    assert e["plan"] == [7, 7, 7, 0, MC_ROW | 0, 1, 2, MC_ROW | 1, 3, 4, 5] + e["store"]
    assert e["res"][5] == 0  # the only marked message hit: nothing for k_msg_roots
    assert exp[1]["res"][9:11] == [2, 0] and exp[1]["pend"] == [] and exp[1]["mcstats"][6] == 2
    assert exp[2]["res"][5] == 0 and exp[3]["res"][5] == 1
    assert exp[4]["res"][8] == 0
    assert exp[5]["res"][9:11] == [1, 1] and exp[5]["pins"] == [0]


# ---------------------------------------------------------------- committees
COMMITTEES = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 65), (0, 33), (1, 7), (1, 450)]


def rbits(n, q=0.5):
    return [1 if _r.random() < q else 0 for _ in range(n)]


def test_bits_sets(driver):
    m = msgs(12)
    bad = [bits_set(m[0], 99, rbits(33)), bits_set(m[1], 5, rbits(33)), bits_set(m[2], 3, rbits(32)),
           Set(msg=m[3], pks=None, pk_len=PK_BITS, n_pks=33)]
    good = [bits_set(m[4 + j], cid, rbits(n, 0.8)) for j, (cid, n) in enumerate([(0, 1), (1, 31), (2, 32), (3, 33), (4, 65)])]
    empty = [bits_set(m[9], 4, [0] * 65), bits_set(m[10], 0, [0])]
    exp = check(driver, [Case(bad + good + empty, COMMITTEES, dedup=True), Case(good, COMMITTEES), Case(bad, COMMITTEES),
                         Case(good[:2] + [keys_set(m[0])] + good[2:], COMMITTEES),
                         Case([bits_set(m[0], 2, [1] * 32), bits_set(m[1], 3, [0] * 32 + [1])], COMMITTEES)])
    assert exp[0]["bits_kerr"] == [BAD_COMMITTEE] * 4 + [0] * 7 and exp[0]["bits_p"][:4] == [0] * 4
    assert exp[0]["bits_p"][9:] == [0, 0] and exp[0]["res"][7] == 1 and exp[3]["res"][7] == 0
    assert exp[4]["sizes"][4] == exp[4]["res"][14] == 3  # every measured word used


def test_multi_sets(driver):
    m = msgs(12)
    cm = COMMITTEES + [(1, 3)] * 64  # ids 8..71: 64 committees of 3
    sets = [
        multi_set(m[0], [], []),                                # k = 0, no member: the identity
        multi_set(m[1], [], [], n_pks=5),                       # k = 0 with members claimed
        multi_set(m[2], list(range(8, 72)), rbits(192, 0.7)),   # k = 64
        Set(msg=m[3], sig=rbytes(96), pks=(65).to_bytes(4, "little"), pk_len=PK_MULTI, n_pks=40),  # refused: no id read
        Set(msg=m[4], sig=rbytes(96), pks=(0xffffffff).to_bytes(4, "little"), pk_len=PK_MULTI, n_pks=40),
        multi_set(m[5], [3, 6], rbits(41)),                     # 33 + 7 != 41
        multi_set(m[6], [3, 5], rbits(66)),                     # an unset committee
        multi_set(m[7], [4, 0, 3], rbits(99, 0.9)),             # good: 3 parts
        bits_set(m[8], 6, rbits(7)),
        keys_set(m[9], 2),
        multi_set(m[10], [4, 6, 3], [0] * 65 + [1] * 7 + [0] * 33),  # parts without a participant are left out
        Set(msg=m[11], sig=rbytes(96), pks=None, pk_len=PK_MULTI, n_pks=0),
        multi_set(m[0], [7, 7], [1] * 449 + [0] + rbits(450, 0.01)),  # a complement part and a direct one
    ]
    exp = check(driver, [Case(sets, cm, dedup=True), Case(sets[7:8], cm), Case(sets[:2], cm)])
    assert exp[0]["bits_kerr"] == [0, BAD_COMMITTEE, 0, BAD_COMMITTEE, BAD_COMMITTEE, BAD_COMMITTEE, BAD_COMMITTEE,
                                   0, 0, 0, 0, BAD_COMMITTEE, 0]
    assert exp[0]["multi_sets"][5 * 8 + 1] == 1 and exp[0]["res"][7] == 0 and exp[1]["res"][7] == 1


# ---------------------------------------------------------------- randomizers
def zero_skipping_seed():
    """a seed whose splitmix64 stream holds a zero early on: splitmix64's output function is a
    bijection of its state, so the state that gives 0 can be computed and a seed placed before it"""
    inv = lambda a: pow(a, -1, 1 << 64)  # noqa: E731

    def unshift(z, s):
        x = z
        for _ in range(64 // s + 1):
            x = z ^ (x >> s)
        return x
    z = unshift(0, 31)
    z = unshift((z * inv(0x94d049bb133111eb)) & M64, 27)
    state = unshift((z * inv(0xbf58476d1ce4e5b9)) & M64, 30)
    return (state - 3 * 0x9e3779b97f4a7c15) & M64  # the third draw is the zero


def test_randomizers(driver):
    m = msgs(6)
    sets = [keys_set(x) for x in m]
    seed0 = zero_skipping_seed()
    g = splitmix(seed0)
    assert [next(g) for _ in range(3)][2] == 0
    with_rnd = [keys_set(x, rnd_in=(1 << 64) - 1 - i) for i, x in enumerate(m)]
    some = [keys_set(x, noscale=int(i in (1, 4))) for i, x in enumerate(m)]
    exp = check(driver, [
        Case(sets, scale=True, seed=1), Case(sets, scale=True, seed=seed0), Case(with_rnd, scale=True, seed=1),
        Case(some, scale=True, seed=1), Case(sets, scale=False, seed=1), Case(some, scale=False),
        # the OS source: fails at once; fails on a redraw; answers zero for set 2 once, then twice more for set 5
        Case(sets, scale=True, entropy=[(0, [])]),
        Case(sets, scale=True, entropy=[(1, [1, 2, 0, 4, 5, 6]), (0, [])]),
        Case(sets, scale=True, entropy=[(1, [1, 2, 0, 4, 5, 0]), (1, [33]), (1, [0]), (1, [0]), (1, [66])]),
        Case(some, scale=True, entropy=[(1, [9, 8, 7, 6, 5, 4])]),
    ])
    g = splitmix(1)
    assert exp[0]["rnd"] == [next(g) for _ in range(6)] and exp[0]["rnd"][0] == 0x910a2dec89025cc1
    assert 0 not in exp[1]["rnd"] and exp[1]["rnd"][:2] == exp[1]["a_rnd"][:2]
    assert exp[2]["rnd"] == [M64 - i for i in range(6)]
    assert [r == 0 for r in exp[3]["rnd"]] == [False, True, False, False, True, False]
    assert exp[4]["rnd"] == [0] * 6 and exp[5]["rnd"] == [0] * 6
    assert exp[6]["rc"] == [ERR_ENTROPY] and exp[7]["rc"] == [ERR_ENTROPY] and exp[7]["entropy_calls"] == [2]
    assert exp[8]["rnd"] == [1, 2, 33, 4, 5, 66] and exp[8]["entropy_calls"] == [5]
    assert exp[9]["rnd"] == [9, 0, 7, 6, 0, 4]


# ---------------------------------------------------------------- layout
LAYOUT_CASES = [(0, 0, 96, 0), (1, 1, 4, 1), (1, 0, 96, 32), (3, 5, 4, 33), (3, 5, 96, 33), (7, 7, 96, 7 * 32),
                (300, 901, 4, 9001), (32768, 32768, 96, 32768 * 32)]


def test_layout(driver):
    got = driver([("layout",) + c for c in LAYOUT_CASES] + [("layout", 300, 901, 96, 9001)])
    for (n, npk, stride, mb), g in zip(LAYOUT_CASES, got):
        off = [int(x) for x in g["layout"]]
        L, size = layout(n, npk, stride, mb)
        names = ["sig", "siglen", "msgoff", "msglen", "mid", "pklen", "rnd", "pk", "msg"]
        assert off == [L[k] for k in names] + [L["bytes"]]
        assert off[0] == 0 and all(o % 8 == 0 for o in off[:9])
        ends = [o + size[k] for o, k in zip(off, names)]
        assert all(e <= o for e, o in zip(ends, off[1:9])), "two fields overlap"
        assert all(o - e < 8 for e, o in zip(ends, off[1:9])), "more than alignment between two fields"
        assert off[9] == ends[-1]
    # the stride-96 layout of the maxima holds any stride-4 layout within them
    big = int(got[-1]["layout"][9])
    for n, npk, mb in [(300, 901, 9001), (299, 901, 9001), (300, 900, 9000), (1, 901, 0), (300, 0, 9001), (0, 0, 0)]:
        assert layout(n, npk, 4, mb)[0]["bytes"] <= big and layout(n, npk, 96, mb)[0]["bytes"] <= big


# ---------------------------------------------------------------- the lists that follow staging
def test_validate_keys_list_and_message_lists(driver):
    m = msgs(4)
    cm = COMMITTEES
    # three jobs, the second not batchable (staged last) and the third flagged: of its index, bits
    # and byte-key sets only the byte keys are listed, in staging order
    sets = [keys_set(m[0], 2), keys_set(m[1]),                                     # job 0: batchable
            keys_set(m[0], 3), index_set(m[1], [4, 5]),                            # job 1: not batchable
            keys_set(m[0], 2), index_set(m[2], [7]), bits_set(m[0], 6, rbits(7, 0.9)), keys_set(m[2], 1, pk_len=96),
            keys_set(m[3], 0)]                                                    # job 2: batchable, flagged
    jobs = [(1, 2), (0, 2), (1 | 4, 5)]
    exp = check(driver, [
        Case(sets, cm, dedup=True, jobs=jobs, lists=(0, 7), scale=True, seed=3, plan_prefix=2),
        Case(sets, cm, dedup=True, jobs=[(1, 2), (0, 2), (1, 5)]),          # no flagged job: nothing listed
        Case(sets, cm, dedup=True, jobs=[(1 | 4, 2), (4, 2), (1, 5)], cache=16),  # a flagged non-batchable job
        Case(sets[5:7], cm, jobs=[(1 | 4, 2)]),                             # flagged, but no byte key
    ])
    e = exp[0]
    # staging order: job 0 (keys 0-2), job 2 (keys 3-4, then 5 and 6), job 1 (keys 7-11)
    assert e["pk_first"] == [0, 2, 3, 5, 6, 6, 7, 7, 10] and e["kv"] == [3, 2]
    assert e["kv_set"] == [0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert e["plan"][2:8] == [3, 4, 6, 2, 2, 5]
    # messages of sets 0..6: m0 m1 m0 m2 m0 m2 m3 -> lists [0 2 4] [1] [3 5] [6]
    assert e["plan"][8:15] == [0, 2, 4, 1, 3, 5, 6] and e["plan"][15:] == [0, 3, 0, 3, 1, 1, 4, 2, 2, 6, 1, 3]
    assert exp[1]["kv"] == [0, 0] and exp[1]["kv_set"] == []
    assert exp[2]["kv"][0] == 2 + 1 + 3 and exp[3]["kv"] == [0, 0] and exp[3]["kv_set"] == []
