"use strict";
/**
 * Committee + bits sets through the real N-API addon on an MI355X (driven by
 * tests/test_gpu_committees.py::test_node_sync_style_package_by_bits, which writes the input
 * file): a sync-aggregate style package -- four subcommittee sets over one message, each given
 * as {committee, bits, bitLen} -- through BlsGpuVerifier.verifySignatureSets, once valid and
 * once with a wrong bit.
 * Run: node tests/js/test_committees_gpu.js <cases.json>
 */
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));

(async () => {
  const pool = new V.BlsGpuVerifier({seed: 7, bufferWaitMs: 5});
  assert.deepStrictEqual(pool.loadPubkeys(0, cases.pks.map(hex)), Array(cases.pks.length).fill(0));
  assert.deepStrictEqual(pool.loadCommittees(cases.first_id, cases.committees), Array(cases.committees.length).fill(0));
  const toSet = (s) => ({committee: s.committee, bits: hex(s.bits), bitLen: s.bit_len, signingRoot: hex(cases.msg), signature: hex(s.sig)});
  const good = cases.sets.map(toSet);
  const forged = good.map((s, i) => (i === cases.wrong.set ? Object.assign({}, s, {bits: hex(cases.wrong.bits)}) : s));
  for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
    assert.strictEqual(await pool.verifySignatureSets(good, opts), true);
    assert.strictEqual(await pool.verifySignatureSets(forged, opts), false);
  }
  // an id nobody loaded: the package's deserializeSet failure
  const unknown = Object.assign({}, good[0], {committee: cases.first_id + 100});
  await assert.rejects(pool.verifySignatureSets([unknown]), /committee/i);
  await pool.close();
  console.log("committees gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
