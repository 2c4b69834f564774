"use strict";
/**
 * Sets spanning several committees through the real N-API addon on an MI355X (driven by
 * tests/test_gpu_committees_multi.py::test_node_electra_style_package, which writes the input
 * file): three aggregates over one message, each given as {committees, bits, bitLen}, through
 * verifySignatureSets of both verifiers and verifySignatureSetsSameMessage, once valid and once
 * with a wrong bit.
 * Run: node tests/js/test_committees_multi_gpu.js <cases.json>
 */
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));

(async () => {
  const toSet = (s) => ({committees: s.committees, bits: hex(s.bits), bitLen: s.bit_len, signingRoot: hex(cases.msg), signature: hex(s.sig)});
  const good = cases.sets.map(toSet);
  const forged = good.map((s, i) => (i === cases.wrong.set ? Object.assign({}, s, {bits: hex(cases.wrong.bits)}) : s));
  const pool = new V.BlsGpuVerifier({seed: 7, bufferWaitMs: 5});
  assert.deepStrictEqual(pool.loadPubkeys(0, cases.pks.map(hex)), Array(cases.pks.length).fill(0));
  assert.deepStrictEqual(pool.loadCommittees(cases.first_id, cases.committees), Array(cases.committees.length).fill(0));
  for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
    assert.strictEqual(await pool.verifySignatureSets(good, opts), true);
    assert.strictEqual(await pool.verifySignatureSets(forged, opts), false);
  }
  // ids as a Uint32Array
  const typed = good.map((s) => Object.assign({}, s, {committees: Uint32Array.from(s.committees)}));
  assert.strictEqual(await pool.verifySignatureSets(typed, {batchable: true}), true);
  // per-set verdicts over the shared message
  const same = (sets) => sets.map((s) => ({committees: s.committees, bits: s.bits, bitLen: s.bitLen, signature: s.signature}));
  assert.deepStrictEqual(await pool.verifySignatureSetsSameMessage(same(good), hex(cases.msg)), good.map(() => true));
  assert.deepStrictEqual(
    await pool.verifySignatureSetsSameMessage(same(forged), hex(cases.msg)),
    good.map((_, i) => i !== cases.wrong.set)
  );
  // an id nobody loaded: the package's deserializeSet failure
  const unknown = Object.assign({}, good[0], {committees: [good[0].committees[0], cases.first_id + 100, good[0].committees[2]]});
  await assert.rejects(pool.verifySignatureSets([unknown]), /committee/i);
  // a bit count that is not the sum of the lengths
  const short = Object.assign({}, good[0], {bitLen: good[0].bitLen - 1});
  await assert.rejects(pool.verifySignatureSets([short]), /committee/i);
  await pool.close();

  const single = new V.BlsGpuSingleThreadVerifier({seed: 7});
  single.addon.pubkeyTableSet(single.ctx, 0, cases.pks.map(hex));
  assert.deepStrictEqual(single.loadCommittees(cases.first_id, cases.committees), Array(cases.committees.length).fill(0));
  assert.strictEqual(await single.verifySignatureSets(good), true);
  assert.strictEqual(await single.verifySignatureSets(forged), false);
  await single.close();
  console.log("committees multi gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
