"use strict";
/**
 * Committee + bits sets of BlsGpuVerifier (lodestar_amd/js/blsGpuVerifier.js) on the CPU, with a
 * fake addon that records what it is given: how a {committee, bits, bitLen} set is packed into
 * the set descriptor and the arena (pk_len 8 = LSG_PK_BITS, n_pks = the bit count, the uint32
 * committee id in host byte order followed by ceil(bitLen / 8) bytes of bits), loadCommittees'
 * argument checks and flattening, and the error against an addon without the entry points.
 * Run: node tests/js/test_committees_host.js   (driven by tests/test_committees_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

function fakeAddon() {
  const m = {
    sets: [], // every set of every package: {pkLen, nPks, keyBytes, msg0}
    committees: [],
    cleared: [],
    open: () => ({ctx: true}),
    close() {},
    slots: () => 2,
    verifyPacked(ctx, arena, setDesc, jobDesc) {
      const nJobs = jobDesc.length / 2;
      let k = 0;
      for (let j = 0; j < nJobs; j++) {
        for (let q = 0; q < jobDesc[2 * j]; q++, k++) {
          const d = setDesc.subarray(7 * k, 7 * k + 7);
          // the bytes lsg_napi.c build_jobs bounds for the set's keys
          const n = d[1] === 8 ? 4 + ((d[2] + 7) >> 3) : d[1] * d[2];
          assert.ok(d[0] + n <= arena.length && d[3] + d[4] <= arena.length && d[5] + d[6] <= arena.length);
          assert.ok(d[0] + n <= d[3], "key bytes run into the message");
          m.sets.push({pkLen: d[1], nPks: d[2], keyBytes: Array.from(arena.subarray(d[0], d[0] + n)), msg0: arena[d[3]]});
        }
      }
      const startNs = Number(process.hrtime.bigint());
      const done = {status: new Uint8Array(nJobs).fill(1), errCode: new Int32Array(nJobs), batchRetries: 0,
                    batchSigsSuccess: 0, startNs, endNs: startNs + 1e6, workerId: 0};
      return new Promise((r) => setTimeout(() => r(done), 1));
    },
    committeesSet(ctx, firstId, indices, offsets) {
      assert.ok(indices instanceof Uint32Array && offsets instanceof Uint32Array);
      m.committees.push({firstId, indices: Array.from(indices), offsets: Array.from(offsets)});
      const err = new Int32Array(offsets.length - 1);
      for (let c = 0; c + 1 < offsets.length; c++) err[c] = offsets[c + 1] === offsets[c] ? 101 : 0;
      return err;
    },
    committeesClear(ctx, firstId, n) {
      m.cleared.push([firstId, n]);
    },
  };
  return m;
}

const root = (id) => new Uint8Array(32).fill(id);
const sig = new Uint8Array(96).fill(1);
const bitsSet = (id, committee, bits, bitLen) => ({committee, bits, bitLen, signingRoot: root(id), signature: sig});
const idBytes = (id) => Array.from(new Uint8Array(new Uint32Array([id]).buffer));

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("a {committee, bits, bitLen} set is packed as id + bits with pk_len 8 and n_pks = bitLen", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
  const wide = new Uint8Array(64).fill(0xff); // a BitArray's buffer may be longer than the field
  wide[1] = 0x81;
  const sets = [
    bitsSet(1, 7, Uint8Array.of(0b10110101), 8),
    bitsSet(2, 0x000f4240 >> 4, Uint8Array.of(0xff, 0x01), 9), // 9 bits: two bytes
    bitsSet(3, (1 << 20) - 1, wide, 450),
    {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.of(5, 6), signingRoot: root(4), signature: sig},
    {type: V.SignatureSetType.single, pubkey: new Uint8Array(48).fill(9), signingRoot: root(5), signature: sig},
    bitsSet(6, 0, new Uint8Array(0), 0),
  ];
  assert.strictEqual(await pool.verifySignatureSets(sets, {batchable: true}), true);
  assert.strictEqual(await pool.verifySignatureSets(sets.slice(0, 2), {verifyOnMainThread: true}), true);
  assert.strictEqual(await pool.verifySignatureSets([sets[2]]), true);
  await pool.close();
  const by = new Map(addon.sets.map((s) => [s.msg0, s]));
  assert.deepStrictEqual(by.get(1), {pkLen: 8, nPks: 8, keyBytes: idBytes(7).concat([0b10110101]), msg0: 1});
  assert.deepStrictEqual(by.get(2), {pkLen: 8, nPks: 9, keyBytes: idBytes(0x000f4240 >> 4).concat([0xff, 0x01]), msg0: 2});
  const s3 = by.get(3);
  assert.deepStrictEqual([s3.pkLen, s3.nPks, s3.keyBytes.length], [8, 450, 4 + 57]);
  assert.deepStrictEqual(s3.keyBytes.slice(0, 6), idBytes((1 << 20) - 1).concat([0xff, 0x81]));
  assert.deepStrictEqual([by.get(4).pkLen, by.get(4).nPks], [4, 2]);
  assert.deepStrictEqual([by.get(5).pkLen, by.get(5).nPks], [48, 1]);
  assert.deepStrictEqual(by.get(6), {pkLen: 8, nPks: 0, keyBytes: idBytes(0), msg0: 6});
  assert.strictEqual(addon.sets.length, 6 + 2 + 1);
});

test("an 8-byte raw key is an unknown key length, never a bits set", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const odd = {type: V.SignatureSetType.single, pubkey: new Uint8Array(8).fill(3), signingRoot: root(1), signature: sig};
  const odds = {type: V.SignatureSetType.aggregate, pubkeys: [new Uint8Array(8), new Uint8Array(8)], signingRoot: root(2), signature: sig};
  await pool.verifySignatureSets([odd, odds]);
  await pool.close();
  assert.deepStrictEqual(addon.sets.map((s) => s.pkLen), [0, 0]);
});

test("malformed bits sets throw at call time", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const bad = [
    bitsSet(1, -1, Uint8Array.of(1), 8),
    bitsSet(1, 1 << 20, Uint8Array.of(1), 8),
    bitsSet(1, 1.5, Uint8Array.of(1), 8),
    bitsSet(1, 3, Uint8Array.of(1), 9), // one byte for nine bits
    bitsSet(1, 3, [1], 8), // not a Uint8Array
    bitsSet(1, 3, Uint8Array.of(1), 131073),
    bitsSet(1, 3, Uint8Array.of(1), undefined),
  ];
  for (const s of bad) await assert.rejects(pool.verifySignatureSets([s], {batchable: true}), /committee|bitLen|bits/);
  assert.strictEqual(addon.sets.length, 0);
  await pool.close();
});

test("getAggregatedPubkeysCount counts the participants of a bits set", async () => {
  const n = V.getAggregatedPubkeysCount([
    bitsSet(1, 7, Uint8Array.of(0xff, 0xff), 9), // 9 of 16 bits count
    bitsSet(2, 7, Uint8Array.of(0b0101, 0xf0), 8),
    {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.of(5, 6, 7)},
    {type: V.SignatureSetType.aggregate, pubkeys: [1, 2]},
    {type: V.SignatureSetType.single, pubkey: 1},
  ]);
  assert.strictEqual(n, 9 + 2 + 3 + 2);
  const inc = [];
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon, metrics: {bls: {aggregatedPubkeys: {inc: (x) => inc.push(x)}}}});
  await pool.verifySignatureSets([bitsSet(1, 7, Uint8Array.of(0b111), 3)]);
  await pool.close();
  assert.deepStrictEqual(inc, [3]);
});

test("loadCommittees flattens its committees, checks its arguments and reports codes", async () => {
  for (const make of [(addon) => new V.BlsGpuVerifier({}, {addon}), (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon})]) {
    const addon = fakeAddon();
    const v = make(addon);
    assert.deepStrictEqual(v.loadCommittees(40, [[3, 1, 1], Uint32Array.of(9), [], [4294967295]]), [0, 0, 101, 0]);
    assert.deepStrictEqual(addon.committees, [{firstId: 40, indices: [3, 1, 1, 9, 4294967295], offsets: [0, 3, 4, 4, 5]}]);
    assert.deepStrictEqual(v.loadCommittees(0, []), []);
    for (const [first, cs, re] of [
      [-1, [[1]], /below 2\^20/],
      [1.5, [[1]], /below 2\^20/],
      [(1 << 20) - 1, [[1], [2]], /below 2\^20/],
      [0, "x", /below 2\^20/],
      [0, [5], /array of validator indices/],
      [0, [[1, -2]], /validator index/],
      [0, [[1, 2.5]], /validator index/],
      [0, [[4294967296]], /validator index/],
      [0, [new Array(131073).fill(1)], /131072/],
    ]) {
      assert.throws(() => v.loadCommittees(first, cs), re);
    }
    assert.strictEqual(addon.committees.length, 2);
    delete addon.committeesSet;
    assert.throws(() => v.loadCommittees(0, [[1]]), /does not support loadCommittees/);
    await v.close();
  }
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  pool.clearCommittees(7, 64);
  assert.deepStrictEqual(addon.cleared, [[7, 64]]);
  delete addon.committeesClear;
  assert.throws(() => pool.clearCommittees(7, 64), /does not support clearCommittees/);
  await pool.close();
});

(async () => {
  let passed = 0;
  for (const t of tests) {
    try {
      await t.fn();
      passed++;
      console.log("ok   " + t.name);
    } catch (e) {
      console.log("FAIL " + t.name + "\n" + (e && e.stack ? e.stack : e));
    }
  }
  console.log(passed + "/" + tests.length + " passed");
  process.exit(passed === tests.length ? 0 : 1);
})();
