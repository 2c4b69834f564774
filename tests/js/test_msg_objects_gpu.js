"use strict";
/**
 * Sets whose message is an SSZ object + domain through the real N-API addon on an MI355X
 * (driven by tests/test_gpu_msg_objects.py::test_node_job_mixing_roots_and_objects, which
 * writes the input file with its expected values): one job mixing signingRoot and
 * signingObject sets -- every object kind, raw keys, pubkeyIndices and {committee, bits,
 * bitLen} -- through BlsGpuVerifier.verifySignatureSets, once valid and once with one object
 * changed; and objectSigningRoots against the expected root.
 * Run: node tests/js/test_msg_objects_gpu.js <cases.json>
 */
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));

function toSet(s) {
  const set = {signature: hex(s.sig)};
  if (s.root !== undefined) set.signingRoot = hex(s.root);
  else Object.assign(set, {signingObject: hex(s.obj), domain: hex(s.domain)});
  if (s.committee !== undefined) return Object.assign(set, {committee: s.committee, bits: hex(s.bits), bitLen: s.bit_len});
  if (s.indices !== undefined) return Object.assign(set, {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.from(s.indices)});
  if (s.pubkeys.length === 1) return Object.assign(set, {type: V.SignatureSetType.single, pubkey: hex(s.pubkeys[0])});
  return Object.assign(set, {type: V.SignatureSetType.aggregate, pubkeys: s.pubkeys.map(hex)});
}

(async () => {
  const pool = new V.BlsGpuVerifier({seed: 7, bufferWaitMs: 5});
  assert.deepStrictEqual(pool.loadPubkeys(0, cases.pks.map(hex)), Array(cases.pks.length).fill(0));
  assert.deepStrictEqual(pool.loadCommittees(cases.committee_id, [cases.committee]), [0]);
  const good = cases.sets.map(toSet);
  assert.ok(good.some((s) => s.signingRoot) && good.some((s) => s.signingObject));
  const forged = good.map((s, i) => (i === cases.forged.set ? Object.assign({}, s, {signingObject: hex(cases.forged.obj)}) : s));
  for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
    assert.strictEqual(await pool.verifySignatureSets(good, opts), true);
    assert.strictEqual(await pool.verifySignatureSets(forged, opts), false);
  }
  // the single-thread verifier (no pubkey table of its own: the sets that carry their keys)
  const own = (s) => s.pubkeyIndices === undefined && s.committee === undefined;
  const single = new V.BlsGpuSingleThreadVerifier({seed: 7});
  assert.strictEqual(await single.verifySignatureSets(good.filter(own)), true);
  assert.strictEqual(await single.verifySignatureSets(forged.filter(own)), false);
  await single.close();
  // the roots-only call of the addon
  const got = pool.addon.objectSigningRoots(pool.ctx, hex(cases.roots.obj), 128, hex(cases.roots.domain));
  assert.strictEqual(Buffer.from(got).toString("hex"), cases.roots.root);
  assert.throws(() => pool.addon.objectSigningRoots(pool.ctx, new Uint8Array(33), 33, hex(cases.roots.domain)), /status 1/);
  await pool.close();
  console.log("msg objects gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
