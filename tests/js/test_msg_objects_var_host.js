"use strict";
/**
 * Variable-size signing objects ({signingObject, domain, signingObjectKind}; a kind tag in the
 * LSG_MSG_OBJECT length word) and the 264-byte ContributionAndProof in BlsGpuVerifier
 * (lodestar_amd/js/blsGpuVerifier.js) on the CPU, with a fake addon that records what it is
 * given: the descriptor's length word is 0x80000000 | tag << 24 | (object + 32), the arena holds
 * the object followed by its domain, malformed objects throw a plain Error before anything is
 * queued on both verifiers, and reserveMsgBytes is passed through.
 * Run: node tests/js/test_msg_objects_var_host.js   (driven by tests/test_msg_objects_var_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const MARK = 0x80000000;
const KIND_MASK = 0x7f000000;

function fakeAddon() {
  const m = {
    jobs: [],
    open: () => ({ctx: true}),
    close() {},
    slots: () => 2,
    verifyPacked(ctx, arena, setDesc, jobDesc) {
      const nJobs = jobDesc.length / 2;
      let k = 0;
      for (let j = 0; j < nJobs; j++) {
        const sets = [];
        for (let q = 0; q < jobDesc[2 * j]; q++, k++) {
          const d = setDesc.subarray(7 * k, 7 * k + 7);
          // the bounds of lsg_napi.c build_jobs: a marked word is marker, tag, payload length
          const keyBytes = d[1] === 8 ? 4 + ((d[2] + 7) >> 3) : d[1] * d[2];
          const msgBytes = d[4] >= MARK ? (d[4] & ~(MARK | KIND_MASK)) >>> 0 : d[4];
          assert.ok(d[0] + keyBytes <= d[3] && d[3] + msgBytes <= d[5] && d[5] + d[6] <= arena.length, "set bytes overlap");
          sets.push({pkLen: d[1], nPks: d[2], lenWord: d[4], msg: Array.from(arena.subarray(d[3], d[3] + msgBytes)), sig0: arena[d[5]]});
        }
        m.jobs.push({sets, flags: jobDesc[2 * j + 1]});
      }
      const startNs = Number(process.hrtime.bigint());
      const done = {status: new Uint8Array(nJobs).fill(1), errCode: new Int32Array(nJobs), batchRetries: 0,
                    batchSigsSuccess: 0, startNs, endNs: startNs + 1e6, workerId: 0};
      return new Promise((r) => setTimeout(() => r(done), 1));
    },
  };
  return m;
}

const KINDS = {AggregateAndProof: {tag: 1, off: 336, maxBytes: 257}, AggregateAndProofElectra: {tag: 2, off: 344, maxBytes: 16385}};
const sig = (id) => new Uint8Array(96).fill(id);
const dom = (id) => Uint8Array.from({length: 32}, (_, i) => (id * 13 + 200 + i) & 255);
const single = (id, msg) => ({type: V.SignatureSetType.single, pubkey: new Uint8Array(48).fill(9), signature: sig(id), ...msg});
const payload = (o, d) => Array.from(o).concat(Array.from(d));
/** a well-formed serialized AggregateAndProof of `nbytes` bitlist bytes whose last byte is `last` */
function agg(kind, nbytes, last, id = 1) {
  const {off} = KINDS[kind];
  const o = Uint8Array.from({length: off + nbytes}, (_, i) => (id * 7 + i) & 255);
  new DataView(o.buffer).setUint32(8, 108, true);
  new DataView(o.buffer).setUint32(108, off - 108, true);
  o[o.length - 1] = last;
  return o;
}
const makers = [(addon, o = {}) => new V.BlsGpuVerifier({bufferWaitMs: 5, ...o}, {addon}), (addon, o = {}) => new V.BlsGpuSingleThreadVerifier(o, {addon})];

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("a tagged object is packed as object || domain with marker and tag in its length word", async () => {
  for (const make of makers) {
    const addon = fakeAddon();
    const v = make(addon);
    const objs = [
      ["AggregateAndProof", agg("AggregateAndProof", 1, 1, 1)],
      ["AggregateAndProof", agg("AggregateAndProof", 57, 0x05, 2)],
      ["AggregateAndProof", agg("AggregateAndProof", 257, 1, 3)],
      ["AggregateAndProofElectra", agg("AggregateAndProofElectra", 1, 0x80, 4)],
      ["AggregateAndProofElectra", agg("AggregateAndProofElectra", 3601, 1, 5)],
      ["AggregateAndProofElectra", agg("AggregateAndProofElectra", 16385, 1, 6)],
    ];
    const sets = objs.map(([kind, o], i) => single(i + 1, {signingObject: o, domain: dom(i), signingObjectKind: kind}));
    sets.push(single(7, {signingObject: new Uint8Array(264).fill(3), domain: dom(7)})); // ContributionAndProof, by length
    sets.push(single(8, {signingRoot: new Uint8Array(32).fill(8)}));
    assert.strictEqual(await v.verifySignatureSets(sets, {batchable: true}), true);
    assert.strictEqual(await v.verifySignatureSets(sets), true); // one job mixing all of them
    await v.close();
    const got = [].concat(...addon.jobs.map((j) => j.sets));
    assert.strictEqual(got.length, 2 * sets.length);
    objs.forEach(([kind, o], i) => {
      const found = got.filter((x) => x.sig0 === i + 1);
      assert.strictEqual(found.length, 2);
      for (const s of found) {
        assert.strictEqual(s.lenWord, (MARK + KINDS[kind].tag * 2 ** 24 + o.length + 32) >>> 0);
        assert.deepStrictEqual(s.msg, payload(o, dom(i)));
      }
    });
    for (const s of got.filter((x) => x.sig0 === 7)) {
      assert.strictEqual(s.lenWord, (MARK | 296) >>> 0);
      assert.deepStrictEqual(s.msg, payload(new Uint8Array(264).fill(3), dom(7)));
    }
    for (const s of got.filter((x) => x.sig0 === 8)) assert.strictEqual(s.lenWord, 32);
    assert.strictEqual(addon.jobs[addon.jobs.length - 1].sets.length, sets.length);
  }
});

test("malformed tagged objects throw a plain Error before anything is queued", async () => {
  for (const make of makers) {
    const addon = fakeAddon();
    const v = make(addon);
    const bad = [];
    for (const kind of Object.keys(KINDS)) {
      const {off, maxBytes} = KINDS[kind];
      const other = kind === "AggregateAndProof" ? "AggregateAndProofElectra" : "AggregateAndProof";
      const m = (o, k = kind) => single(1, {signingObject: o, domain: dom(1), signingObjectKind: k});
      const o1 = agg(kind, 33, 0x1f);
      o1[8] ^= 1; // the outer offset
      const o2 = agg(kind, 33, 0x1f);
      o2[108] ^= 8; // the inner offset
      const o3 = agg(kind, 33, 0x1f);
      o3[111] = 1; // its high byte
      bad.push(m(o1), m(o2), m(o3));
      bad.push(m(agg(kind, 33, 0)), m(agg(kind, 1, 0))); // a zero last byte
      bad.push(m(agg(kind, maxBytes, 2)), m(agg(kind, maxBytes, 0x80))); // more bits than the limit
      bad.push(m(agg(kind, maxBytes + 1, 1))); // a byte too long
      bad.push(m(agg(kind, 33, 0x1f).subarray(0, off)), m(new Uint8Array(4))); // no bitlist byte
      bad.push(m(agg(kind, 33, 0x1f), other)); // the other kind's layout
      bad.push(m(agg(kind, 33, 0x1f), "Attestation"), m(agg(kind, 33, 0x1f), "toString"), m(agg(kind, 33, 0x1f), 1)); // unknown kinds
      bad.push(m(Array.from(agg(kind, 33, 0x1f)))); // not a Uint8Array
      bad.push(single(1, {signingObject: agg(kind, 33, 0x1f), signingObjectKind: kind})); // no domain
      bad.push(single(1, {signingObject: agg(kind, 33, 0x1f), domain: dom(1)})); // no kind: the length names none
      // the well-formed twins pass
      for (const o of [agg(kind, 33, 0x1f), agg(kind, 1, 1), agg(kind, maxBytes, 1), agg(kind, maxBytes - 1, 0xff)]) {
        assert.strictEqual(await v.verifySignatureSets([m(o)], {batchable: true}), true);
      }
    }
    const before = addon.jobs.length;
    for (const s of bad) {
      for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
        await assert.rejects(v.verifySignatureSets([s], opts), (e) => e.constructor === Error && /signingObject|domain/.test(e.message));
      }
    }
    const good = single(2, {signingObject: agg("AggregateAndProof", 9, 1), domain: dom(2), signingObjectKind: "AggregateAndProof"});
    await assert.rejects(v.verifySignatureSets([good, bad[0], good], {batchable: true}), /signingObject/);
    assert.strictEqual(addon.jobs.length, before);
    assert.strictEqual(await v.verifySignatureSets([good]), true);
    await v.close();
  }
});

test("reserveMsgBytes is passed through for tagged payloads", async () => {
  const calls = [];
  const addon = Object.assign(fakeAddon(), {reserve: (ctx, ...a) => calls.push(a)});
  await new V.BlsGpuVerifier({reserveSets: 100, reservePubkeys: 300, reserveMsgBytes: 100 * 16761}, {addon}).close();
  assert.deepStrictEqual(calls, [[100, 300, 1676100, 2]]);
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
