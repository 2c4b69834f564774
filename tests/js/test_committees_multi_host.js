"use strict";
/**
 * Sets spanning several committees ({committees, bits, bitLen}; LSG_PK_BITS_MULTI) of
 * BlsGpuVerifier and BlsGpuSingleThreadVerifier (lodestar_amd/js/blsGpuVerifier.js) on the CPU,
 * with a fake addon that records what it is given: the set descriptor (pk_len 12, n_pks = the
 * bit count) and the key blob (uint32 count, the uint32 committee ids in host byte order,
 * ceil(bitLen / 8) bytes of bits), the call-time checks, the mapping of a 12-byte raw key to
 * an unknown key length, the participant count, and verifySignatureSetsSameMessage passing the
 * form through.
 * Run: node tests/js/test_committees_multi_host.js  (driven by tests/test_committees_multi_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

function fakeAddon() {
  const m = {
    sets: [], // every set of every package: {pkLen, nPks, keyBytes, msg0}
    open: () => ({ctx: true}),
    close() {},
    slots: () => 2,
    verifyPacked(ctx, arena, setDesc, jobDesc) {
      const nJobs = jobDesc.length / 2;
      let k = 0;
      for (let j = 0; j < nJobs; j++) {
        for (let q = 0; q < jobDesc[2 * j]; q++, k++) {
          const d = setDesc.subarray(7 * k, 7 * k + 7);
          // the bytes lsg_napi.c build_jobs bounds for the set's keys: a multi set's from the
          // blob's own leading count
          let n = d[1] * d[2];
          if (d[1] === 8) n = 4 + ((d[2] + 7) >> 3);
          if (d[1] === 12) {
            assert.ok(d[0] + 4 <= arena.length);
            const cnt = new Uint32Array(arena.slice(d[0], d[0] + 4).buffer)[0];
            n = 4 + 4 * cnt + ((d[2] + 7) >> 3);
          }
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
  };
  return m;
}

const root = (id) => new Uint8Array(32).fill(id);
const sig = new Uint8Array(96).fill(1);
const multiSet = (id, committees, bits, bitLen) => ({committees, bits, bitLen, signingRoot: root(id), signature: sig});
const words = (...w) => Array.from(new Uint8Array(new Uint32Array(w).buffer));

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("a {committees, bits, bitLen} set is packed as count + ids + bits with pk_len 12 and n_pks = bitLen", async () => {
  for (const make of [(addon) => new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon}), (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon})]) {
    const addon = fakeAddon();
    const v = make(addon);
    const wide = new Uint8Array(4000).fill(0xff); // a BitArray's buffer may be longer than the field
    wide[1] = 0x81;
    const ids64 = Array.from({length: 64}, (_, c) => (1 << 20) - 1 - c);
    const sets = [
      multiSet(1, [7, 3], Uint8Array.of(0b10110101, 0x01), 9),
      multiSet(2, Uint32Array.of(5, 5, 0x000f4240 >> 4), Uint8Array.of(0xff, 0x01, 0xee), 17), // 17 bits: three bytes
      multiSet(3, ids64, wide, 28801),
      {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.of(5, 6), signingRoot: root(4), signature: sig},
      {committee: 9, bits: Uint8Array.of(3), bitLen: 2, signingRoot: root(5), signature: sig},
      multiSet(6, [], new Uint8Array(0), 0),
      multiSet(7, [4], Uint8Array.of(0xff), 3),
    ];
    assert.strictEqual(await v.verifySignatureSets(sets, {batchable: true}), true);
    assert.strictEqual(await v.verifySignatureSets(sets.slice(0, 2), {verifyOnMainThread: true}), true);
    await v.close();
    const by = new Map(addon.sets.slice(0, 7).map((s) => [s.msg0, s]));
    assert.deepStrictEqual(by.get(1), {pkLen: 12, nPks: 9, keyBytes: words(2, 7, 3).concat([0b10110101, 0x01]), msg0: 1});
    assert.deepStrictEqual(by.get(2), {pkLen: 12, nPks: 17, keyBytes: words(3, 5, 5, 0x000f4240 >> 4).concat([0xff, 0x01, 0xee]), msg0: 2});
    const s3 = by.get(3);
    assert.deepStrictEqual([s3.pkLen, s3.nPks, s3.keyBytes.length], [12, 28801, 4 + 256 + 3601]);
    assert.deepStrictEqual(s3.keyBytes.slice(0, 4 + 256 + 2), words(64, ...ids64).concat([0xff, 0x81]));
    assert.deepStrictEqual([by.get(4).pkLen, by.get(4).nPks], [4, 2]);
    assert.deepStrictEqual([by.get(5).pkLen, by.get(5).nPks], [8, 2]);
    assert.deepStrictEqual(by.get(6), {pkLen: 12, nPks: 0, keyBytes: words(0), msg0: 6});
    assert.deepStrictEqual(by.get(7), {pkLen: 12, nPks: 3, keyBytes: words(1, 4).concat([0xff]), msg0: 7});
    assert.strictEqual(addon.sets.length, 7 + 2);
    assert.deepStrictEqual(addon.sets.slice(7).map((s) => [s.pkLen, s.nPks]), [[12, 9], [12, 17]]);
  }
});

test("a 12-byte raw key is an unknown key length, never a multi set", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const odd = {type: V.SignatureSetType.single, pubkey: new Uint8Array(12).fill(3), signingRoot: root(1), signature: sig};
  const odds = {type: V.SignatureSetType.aggregate, pubkeys: [new Uint8Array(12), new Uint8Array(12)], signingRoot: root(2), signature: sig};
  await pool.verifySignatureSets([odd, odds]);
  await pool.verifySignatureSetsSameMessage([{publicKey: new Uint8Array(12).fill(3), signature: sig}], root(3));
  await pool.close();
  assert.deepStrictEqual(addon.sets.map((s) => s.pkLen), [0, 0, 0]);
});

test("malformed multi sets throw at call time", async () => {
  for (const make of [(addon) => new V.BlsGpuVerifier({}, {addon}), (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon})]) {
    const addon = fakeAddon();
    const v = make(addon);
    const bad = [
      multiSet(1, [3, -1], Uint8Array.of(1), 8),
      multiSet(1, [1 << 20], Uint8Array.of(1), 8),
      multiSet(1, [1.5], Uint8Array.of(1), 8),
      multiSet(1, 3, Uint8Array.of(1), 8), // not a list
      multiSet(1, new Array(65).fill(2), Uint8Array.of(1), 8), // more than 64 committees
      multiSet(1, [3, 4], Uint8Array.of(1), 9), // one byte for nine bits
      multiSet(1, [3], [1], 8), // not a Uint8Array
      multiSet(1, [3], Uint8Array.of(1), -1),
      multiSet(1, [3], Uint8Array.of(1), undefined),
    ];
    for (const s of bad) await assert.rejects(v.verifySignatureSets([s], {batchable: true}), /committee|bitLen|bits/);
    assert.strictEqual(addon.sets.length, 0);
    await v.close();
  }
});

test("getAggregatedPubkeysCount counts the participants of a multi set", async () => {
  const n = V.getAggregatedPubkeysCount([
    multiSet(1, [7, 8], Uint8Array.of(0xff, 0xff), 9), // 9 of 16 bits count
    multiSet(2, [7], Uint8Array.of(0b0101, 0xf0), 8),
    {committee: 1, bits: Uint8Array.of(0b11), bitLen: 2},
    {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.of(5, 6, 7)},
  ]);
  assert.strictEqual(n, 9 + 2 + 2 + 3);
  const inc = [];
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon, metrics: {bls: {aggregatedPubkeys: {inc: (x) => inc.push(x)}}}});
  await pool.verifySignatureSets([multiSet(1, [7, 9], Uint8Array.of(0b111), 3)]);
  await pool.close();
  assert.deepStrictEqual(inc, [3]);
});

test("verifySignatureSetsSameMessage passes a multi set through", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
  const got = await pool.verifySignatureSetsSameMessage(
    [
      {committees: [2, 9], bits: Uint8Array.of(0x0f, 0x02), bitLen: 10, signature: sig},
      {publicKey: new Uint8Array(48).fill(9), signature: sig},
      {committees: [2], bits: Uint8Array.of(1), bitLen: 9, signature: sig}, // malformed: false, as any failing set
    ],
    root(8)
  );
  await pool.close();
  assert.deepStrictEqual(got, [true, true, false]);
  assert.deepStrictEqual(
    addon.sets.map((s) => [s.pkLen, s.nPks, s.msg0]),
    [[12, 10, 8], [48, 1, 8]]
  );
  assert.deepStrictEqual(addon.sets[0].keyBytes, words(2, 2, 9).concat([0x0f, 0x02]));
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
