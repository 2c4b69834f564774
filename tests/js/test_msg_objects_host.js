"use strict";
/**
 * Sets whose message is an SSZ object + domain ({signingObject, domain}, LSG_MSG_OBJECT) in
 * BlsGpuVerifier (lodestar_amd/js/blsGpuVerifier.js) on the CPU, with a fake addon that records
 * what it is given: the descriptor's length word is 0x80000000 | (object + 32), the arena holds
 * the object followed by its domain, object and root sets share a job, every key form takes
 * the message form, and malformed objects throw before anything is queued.
 * Run: node tests/js/test_msg_objects_host.js   (driven by tests/test_msg_objects_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const MARK = 0x80000000;

function fakeAddon() {
  const m = {
    jobs: [], // per package job: its sets {pkLen, nPks, lenWord, msg: number[], sig0}
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
          // the bounds of lsg_napi.c build_jobs: the message's bytes are the masked length
          const keyBytes = d[1] === 8 ? 4 + ((d[2] + 7) >> 3) : d[1] * d[2];
          const msgBytes = (d[4] & ~MARK) >>> 0;
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

const LENGTHS = [8, 16, 32, 76, 88, 112, 128];
const sig = (id) => new Uint8Array(96).fill(id);
const obj = (len, id) => Uint8Array.from({length: len}, (_, i) => (id * 7 + i) & 255);
const dom = (id) => Uint8Array.from({length: 32}, (_, i) => (id * 13 + 200 + i) & 255);
const single = (id, msg) => ({type: V.SignatureSetType.single, pubkey: new Uint8Array(48).fill(9), signature: sig(id), ...msg});
const payload = (o, d) => Array.from(o).concat(Array.from(d));

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("an object set is packed as object || domain with the marker in its length word", async () => {
  for (const make of [(addon) => new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon}), (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon})]) {
    const addon = fakeAddon();
    const v = make(addon);
    const sets = LENGTHS.map((len, i) => single(i + 1, {signingObject: obj(len, i), domain: dom(i)}));
    assert.strictEqual(await v.verifySignatureSets(sets, {batchable: true}), true);
    await v.close();
    const got = [].concat(...addon.jobs.map((j) => j.sets));
    assert.strictEqual(got.length, LENGTHS.length);
    LENGTHS.forEach((len, i) => {
      const s = got.find((x) => x.sig0 === i + 1);
      assert.strictEqual(s.lenWord, (MARK | (len + 32)) >>> 0);
      assert.deepStrictEqual(s.msg, payload(obj(len, i), dom(i)));
      assert.deepStrictEqual([s.pkLen, s.nPks], [48, 1]);
    });
  }
});

test("object and root sets share one job", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const root = new Uint8Array(32).fill(0x55);
  const sets = [
    single(1, {signingRoot: root}),
    single(2, {signingObject: obj(128, 2), domain: dom(2)}),
    single(3, {signingRoot: new Uint8Array(0)}),
    single(4, {signingObject: obj(8, 4), domain: dom(4)}),
  ];
  assert.strictEqual(await pool.verifySignatureSets(sets), true);
  await pool.close();
  assert.strictEqual(addon.jobs.length, 1);
  const s = addon.jobs[0].sets;
  assert.deepStrictEqual(s.map((x) => x.lenWord), [32, (MARK | 160) >>> 0, 0, (MARK | 40) >>> 0]);
  assert.deepStrictEqual(s[0].msg, Array.from(root));
  assert.deepStrictEqual(s[1].msg, payload(obj(128, 2), dom(2)));
  assert.deepStrictEqual(s[3].msg, payload(obj(8, 4), dom(4)));
});

test("every key form takes an object message", async () => {
  for (const opts of [{batchable: true}, {verifyOnMainThread: true}, {}]) {
    const addon = fakeAddon();
    const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
    const m = (id) => ({signingObject: obj(128, id), domain: dom(id), signature: sig(id)});
    const sets = [
      {type: V.SignatureSetType.single, pubkey: new Uint8Array(96).fill(1), ...m(1)},
      {type: V.SignatureSetType.single, pubkey: {toBytes: () => new Uint8Array(96).fill(2)}, ...m(2)},
      {type: V.SignatureSetType.aggregate, pubkeys: [new Uint8Array(48), new Uint8Array(48), new Uint8Array(48)], ...m(3)},
      {type: V.SignatureSetType.aggregate, pubkeyIndices: Uint32Array.of(5, 6), ...m(4)},
      {committee: 7, bits: Uint8Array.of(0xff, 0x01), bitLen: 9, ...m(5)},
    ];
    assert.strictEqual(await pool.verifySignatureSets(sets, opts), true);
    await pool.close();
    const got = [].concat(...addon.jobs.map((j) => j.sets));
    assert.deepStrictEqual(got.map((x) => [x.pkLen, x.nPks]), [[96, 1], [96, 1], [48, 3], [4, 2], [8, 9]]);
    got.forEach((s, i) => {
      assert.strictEqual(s.lenWord, (MARK | 160) >>> 0);
      assert.deepStrictEqual(s.msg, payload(obj(128, i + 1), dom(i + 1)));
    });
  }
});

test("a long package of object sets outgrows the arena's estimate", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const sets = Array.from({length: 100}, (_, i) => single(1 + (i % 200), {signingObject: obj(128, i), domain: dom(i)}));
  assert.strictEqual(await pool.verifySignatureSets(sets), true);
  await pool.close();
  const got = [].concat(...addon.jobs.map((j) => j.sets));
  assert.strictEqual(got.length, 100);
  got.forEach((s, i) => assert.deepStrictEqual(s.msg, payload(obj(128, i), dom(i))));
});

test("reserveMsgBytes sizes the reservation's message bytes; the default stays 32 per set", async () => {
  const calls = [];
  const addon = Object.assign(fakeAddon(), {reserve: (ctx, ...a) => calls.push(a)});
  await new V.BlsGpuVerifier({reserveSets: 1000}, {addon}).close();
  await new V.BlsGpuVerifier({reserveSets: 1000, reservePubkeys: 5000, reserveMsgBytes: 160000}, {addon}).close();
  await new V.BlsGpuVerifier({reserveMsgBytes: 160000}, {addon}).close(); // no reserveSets: no reservation
  assert.deepStrictEqual(calls, [[1000, 1000, 32000, 2], [1000, 5000, 160000, 2]]);
});

test("malformed objects and domains throw a plain Error before anything is queued", async () => {
  for (const make of [(addon) => new V.BlsGpuVerifier({}, {addon}), (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon})]) {
    const addon = fakeAddon();
    const v = make(addon);
    const bad = [];
    for (let len = 0; len <= 200; len++) if (!LENGTHS.includes(len)) bad.push(single(1, {signingObject: new Uint8Array(len), domain: dom(1)}));
    bad.push(single(1, {signingObject: Array.from(obj(32, 1)), domain: dom(1)})); // not a Uint8Array
    bad.push(single(1, {signingObject: obj(32, 1)})); // no domain
    bad.push(single(1, {signingObject: obj(32, 1), domain: new Uint8Array(31)}));
    bad.push(single(1, {signingObject: obj(32, 1), domain: new Uint8Array(33)}));
    bad.push(single(1, {signingObject: obj(32, 1), domain: Array.from(dom(1))}));
    for (const s of bad) {
      for (const opts of [{batchable: true}, {}, {verifyOnMainThread: true}]) {
        await assert.rejects(v.verifySignatureSets([s], opts), (e) => e.constructor === Error && /signingObject|domain/.test(e.message));
      }
    }
    // one bad set among good ones rejects the call, and nothing of it reaches the addon
    const good = single(2, {signingObject: obj(16, 2), domain: dom(2)});
    await assert.rejects(v.verifySignatureSets([good, bad[0], good], {batchable: true}), /signingObject/);
    assert.strictEqual(addon.jobs.length, 0);
    assert.strictEqual(await v.verifySignatureSets([good]), true);
    await v.close();
  }
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
