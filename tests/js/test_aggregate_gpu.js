"use strict";
/**
 * options.onAggregates through the real N-API addon on an MI355X (driven by
 * tests/test_gpu_sig_groups.py::test_node_handler_gets_the_aggregates, which writes the input
 * file): single-set batchable calls carrying aggregateKey / aggregateTag, some forged, some
 * without a key.  Per key, the handler's entries -- one per package that held verified sets of
 * the key -- must sum to aggregateSignatures over the sets that resolved true, their counts and
 * tags must be those sets', and a priority call holding a signature and its negative must give
 * the point at infinity with count 2.
 * Run: node tests/js/test_aggregate_gpu.js <cases.json>
 */
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const toHex = (b) => Buffer.from(b).toString("hex");
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));

(async () => {
  const entries = [];
  let settled = 0;
  let settledAtHandler = -1;
  const pool = new V.BlsGpuVerifier({
    seed: 7,
    bufferWaitMs: 5,
    onAggregates: (e) => {
      if (settledAtHandler < 0) settledAtHandler = settled;
      entries.push(...e);
    },
  });
  const toSet = (s) => {
    const set = {type: V.SignatureSetType.single, pubkey: hex(s.pk), signingRoot: hex(s.msg), signature: hex(s.sig)};
    if (s.key !== null) {
      set.aggregateKey = s.key;
      set.aggregateTag = s.tag;
    }
    return set;
  };
  const verdicts = await Promise.all(
    cases.sets.map((s) =>
      pool.verifySignatureSets([toSet(s)], {batchable: true}).then((v) => {
        settled++;
        return v;
      })
    )
  );
  assert.deepStrictEqual(verdicts.map((v, i) => (v ? -1 : i)).filter((i) => i >= 0), cases.forged);
  assert.strictEqual(settledAtHandler, 0, "the first handler call came before any verdict");
  // per key: the verified sets
  const want = new Map();
  cases.sets.forEach((s, i) => {
    if (s.key === null || !verdicts[i]) return;
    if (!want.has(s.key)) want.set(s.key, {sigs: [], tags: []});
    want.get(s.key).sigs.push(hex(s.sig96));
    want.get(s.key).tags.push(s.tag);
  });
  const got = new Map();
  for (const e of entries) {
    assert.ok(e.signature instanceof Uint8Array && e.signature.length === 96 && e.count > 0 && e.tags.length === e.count);
    if (!got.has(e.key)) got.set(e.key, {sigs: [], tags: [], count: 0});
    const g = got.get(e.key);
    g.sigs.push(e.signature);
    g.tags.push(...e.tags);
    g.count += e.count;
  }
  assert.deepStrictEqual(Array.from(got.keys()).sort(), Array.from(want.keys()).sort());
  const keys = Array.from(want.keys());
  const expect = pool.aggregateSignatures(keys.map((k) => want.get(k).sigs));
  const merged = pool.aggregateSignatures(keys.map((k) => got.get(k).sigs));
  keys.forEach((k, i) => {
    assert.strictEqual(expect[i].err, 0);
    assert.strictEqual(toHex(merged[i].signature), toHex(expect[i].signature), k);
    assert.strictEqual(got.get(k).count, want.get(k).sigs.length, k);
    assert.deepStrictEqual(got.get(k).tags.slice().sort((a, b) => a - b), want.get(k).tags.slice().sort((a, b) => a - b), k);
  });
  // one priority job: a signature and its negative under one key
  entries.length = 0;
  const pair = cases.sets.filter((s) => s.key === cases.cancel_key).map(toSet);
  assert.strictEqual(pair.length, 2);
  assert.strictEqual(await pool.verifySignatureSets(pair, {verifyOnMainThread: true}), true);
  assert.strictEqual(entries.length, 1);
  assert.strictEqual(toHex(entries[0].signature), "c0" + "00".repeat(95));
  assert.deepStrictEqual([entries[0].key, entries[0].count, entries[0].tags.length], [cases.cancel_key, 2, 2]);
  await pool.close();
  console.log("aggregate gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
