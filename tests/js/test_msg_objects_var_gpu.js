"use strict";
/**
 * Tagged signing objects through the real N-API addon on an MI355X (driven by
 * tests/test_gpu_msg_objects_var.py::test_node_job_mixing_roots_fixed_and_tagged_objects, which
 * writes the input file with its expected values): one job mixing signingRoot sets, fixed-size
 * signingObject sets (the 264-byte ContributionAndProof among them) and AggregateAndProof
 * objects of both kinds -- raw keys and pubkeyIndices -- through verifySignatureSets on both
 * verifiers, once valid and once with a participation bit of one signed object flipped; a
 * malformed object throws at call time; and objectSigningRootsVar against the expected roots.
 * Run: node tests/js/test_msg_objects_var_gpu.js <cases.json>
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
  if (s.kind !== undefined) set.signingObjectKind = s.kind;
  if (s.indices !== undefined) return Object.assign(set, {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.from(s.indices)});
  return Object.assign(set, {type: V.SignatureSetType.single, pubkey: hex(s.pubkeys[0])});
}

(async () => {
  const pool = new V.BlsGpuVerifier({seed: 7, bufferWaitMs: 5, reserveSets: 64, reservePubkeys: 256, reserveMsgBytes: cases.reserve_msg_bytes});
  assert.deepStrictEqual(pool.loadPubkeys(0, cases.pks.map(hex)), Array(cases.pks.length).fill(0));
  const good = cases.sets.map(toSet);
  assert.ok(good.some((s) => s.signingRoot) && good.some((s) => s.signingObject && !s.signingObjectKind));
  assert.ok(good.some((s) => s.signingObjectKind === "AggregateAndProof") && good.some((s) => s.signingObjectKind === "AggregateAndProofElectra"));
  const forged = good.map((s, i) => (i === cases.forged.set ? Object.assign({}, s, {signingObject: hex(cases.forged.obj)}) : s));
  for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
    assert.strictEqual(await pool.verifySignatureSets(good, opts), true);
    assert.strictEqual(await pool.verifySignatureSets(forged, opts), false);
  }
  // a malformed object is refused at call time, and the verifier goes on working
  const tagged = good.findIndex((s) => s.signingObjectKind !== undefined);
  const zeroLast = Uint8Array.from(good[tagged].signingObject);
  zeroLast[zeroLast.length - 1] = 0;
  const bad = good.map((s, i) => (i === tagged ? Object.assign({}, s, {signingObject: zeroLast}) : s));
  await assert.rejects(pool.verifySignatureSets(bad, {batchable: true}), (e) => e.constructor === Error && /delimiter/.test(e.message));
  assert.strictEqual(await pool.verifySignatureSets(good), true);
  // the single-thread verifier (no pubkey table of its own: the sets that carry their keys)
  const own = (s) => s.pubkeyIndices === undefined;
  const single = new V.BlsGpuSingleThreadVerifier({seed: 7});
  assert.strictEqual(await single.verifySignatureSets(good.filter(own)), true);
  assert.strictEqual(await single.verifySignatureSets(forged.filter(own)), false);
  await single.close();
  // the roots-only call of the addon
  for (const r of cases.roots) {
    const objs = r.objs.map(hex);
    const offsets = new Uint32Array(objs.length + 1);
    objs.forEach((o, i) => (offsets[i + 1] = offsets[i] + o.length));
    const all = new Uint8Array(offsets[objs.length]);
    objs.forEach((o, i) => all.set(o, offsets[i]));
    const got = pool.addon.objectSigningRootsVar(pool.ctx, r.tag, all, offsets, hex(r.domain));
    assert.strictEqual(Buffer.from(got).toString("hex"), r.roots.join(""));
    assert.throws(() => pool.addon.objectSigningRootsVar(pool.ctx, 3 - r.tag, all, offsets, hex(r.domain)), /status 1/);
    assert.throws(() => pool.addon.objectSigningRootsVar(pool.ctx, r.tag, all, offsets.subarray(1), hex(r.domain)), TypeError);
  }
  await pool.close();
  console.log("msg objects var gpu ok");
})().catch((e) => {
  console.log(e && e.stack ? e.stack : e);
  process.exit(1);
});
