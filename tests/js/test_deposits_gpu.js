"use strict";
/**
 * Objects that carry their own keys, through the real N-API addon on an MI355X (driven by
 * tests/test_gpu_validate_keys.py::test_node_deposits_and_validate_on_gpu, which writes the
 * input file with oracle-made sets and codes): verifyDeposits over the oracle's deposit fixture
 * (tests/golden/deposits.json; its first case is the genesis known answer), a flagged
 * verifySignatureSets that rejects an alias key pk + T the unflagged call accepts, and the
 * addon's pubkeyValidate.
 * Run: node tests/js/test_deposits_gpu.js <cases.json>
 */
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const gold = JSON.parse(fs.readFileSync(path.join(__dirname, "..", "golden", "deposits.json"), "utf8")).cases;
const toSet = (c) => ({type: V.SignatureSetType.single, pubkey: hex(c.pk), signingRoot: hex(c.msg), signature: hex(c.sig)});

(async () => {
  const pool = new V.BlsGpuVerifier({seed: 7, bufferWaitMs: 5});
  const domain = hex(gold[0].domain);
  // the genesis known answer alone, then every fixture case in one call
  assert.deepStrictEqual(await pool.verifyDeposits([hex(gold[0].data)], domain), [true]);
  assert.deepStrictEqual(await pool.verifyDeposits(gold.map((c) => hex(c.data)), domain), gold.map((c) => c.valid === 1));
  const raw = pool.addon.verifyDeposits(pool.ctx, hex(gold.map((c) => c.data).join("")), domain);
  assert.deepStrictEqual(Array.from(raw.valid), gold.map((c) => c.valid));
  assert.deepStrictEqual(Array.from(raw.err), gold.map((c) => c.err));
  // the alias key: accepted unflagged (as the oracle's plain verify says), rejected flagged,
  // without touching the jobs batched with it
  const good = toSet(cases.good);
  const alias = toSet(cases.alias);
  for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
    const unflagged = pool.verifySignatureSets([alias], opts);
    const flagged = pool.verifySignatureSets([alias], Object.assign({validatePubkeys: true}, opts));
    const others = [pool.verifySignatureSets([good], Object.assign({validatePubkeys: true}, opts)), pool.verifySignatureSets([good], opts)];
    await assert.rejects(flagged, /BLST_POINT_NOT_IN_GROUP/);
    assert.strictEqual(await unflagged, cases.alias_unvalidated);
    assert.deepStrictEqual(await Promise.all(others), [true, true]);
  }
  // batched KeyValidate, which the addon now exposes
  assert.deepStrictEqual(Array.from(pool.addon.pubkeyValidate(pool.ctx, hex(cases.keys.pks), 96)), cases.keys.err);
  await pool.close();
  console.log("deposits gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
