"use strict";
/**
 * opts.validatePubkeys and verifyDeposits of BlsGpuVerifier (lodestar_amd/js/blsGpuVerifier.js)
 * on the CPU, with a fake addon that records every package's job descriptors: the
 * LSG_JOB_VALIDATE_KEYS bit (4) must reach the descriptor of exactly the flagged calls' jobs
 * when flagged and unflagged calls are interleaved, buffered, queued and sent directly.
 * The fake's verdict rule is a toy: a flagged job whose key starts with 0xBA is LSG_ERROR with
 * BLST_POINT_NOT_IN_GROUP (3); every other job is valid.
 * Run: node tests/js/test_validate_host.js   (driven by tests/test_validate_keys_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const VALIDATE = 4;

function fakeAddon() {
  const m = {
    jobs: [], // every job of every package: {id, flags, pk0, priority}
    packages: 0,
    deposits: [],
    open: () => ({ctx: true}),
    close() {},
    slots: () => 2,
    verifyPacked(ctx, arena, setDesc, jobDesc, seed, priority) {
      m.packages++;
      const status = new Uint8Array(jobDesc.length / 2);
      const errCode = new Int32Array(jobDesc.length / 2);
      let k = 0;
      for (let j = 0; j < jobDesc.length / 2; j++) {
        const flags = jobDesc[2 * j + 1];
        let st = 1;
        for (let q = 0; q < jobDesc[2 * j]; q++, k++) {
          const d = setDesc.subarray(7 * k, 7 * k + 7);
          const rec = {id: arena[d[3]] | (arena[d[3] + 1] << 8), flags, pk0: arena[d[0]], priority: !!priority, package: m.packages};
          m.jobs.push(rec);
          if (flags & VALIDATE && rec.pk0 === 0xba) st = 2;
        }
        status[j] = st;
        errCode[j] = st === 2 ? 3 : 0;
      }
      const startNs = Number(process.hrtime.bigint());
      const done = {status, errCode, batchRetries: 0, batchSigsSuccess: 0, startNs, endNs: startNs + 1e6, workerId: 0};
      return new Promise((r) => setTimeout(() => r(done), 1));
    },
    verifyDeposits(ctx, data, domain) {
      m.deposits.push({n: data.length / 184, domain: Buffer.from(domain).toString("hex")});
      const n = data.length / 184;
      const valid = new Uint8Array(n);
      const err = new Int32Array(n);
      for (let i = 0; i < n; i++) {
        valid[i] = data[184 * i] === 0xba ? 0 : 1;
        err[i] = data[184 * i] === 0xba ? 3 : 0;
      }
      return {valid, err};
    },
  };
  return m;
}

/** set `id` (carried in the first two message bytes); badKey: its key starts with 0xBA */
function set(id, badKey = false) {
  const message = new Uint8Array(32);
  message[0] = id & 255;
  message[1] = id >> 8;
  return {type: V.SignatureSetType.single, pubkey: new Uint8Array(48).fill(badKey ? 0xba : 7), signingRoot: message,
          signature: new Uint8Array(96).fill(1)};
}

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("validatePubkeys reaches exactly the flagged calls' job descriptors (interleaved, buffered)", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
  const flagged = new Set();
  const ps = [];
  let id = 0;
  // buffered batchable calls, alternating and in runs; non-batchable and priority calls between
  const kinds = [true, false, true, true, false, false, true, false, true, true, true, false];
  for (let round = 0; round < 8; round++) {
    for (const f of kinds) {
      const opts = {batchable: true};
      if (f) opts.validatePubkeys = true;
      if (f) flagged.add(id);
      ps.push(pool.verifySignatureSets([set(id++)], opts));
    }
    flagged.add(id);
    ps.push(pool.verifySignatureSets([set(id++)], {validatePubkeys: true})); // queued, not buffered
    ps.push(pool.verifySignatureSets([set(id++)], {}));
    flagged.add(id);
    ps.push(pool.verifySignatureSets([set(id++)], {validatePubkeys: true, priority: true}));
    ps.push(pool.verifySignatureSets([set(id++)], {priority: true, batchable: true}));
    flagged.add(id);
    ps.push(pool.verifySignatureSets([set(id++)], {validatePubkeys: true, verifyOnMainThread: true}));
    ps.push(pool.verifySignatureSets([set(id++)], {verifyOnMainThread: true}));
  }
  // a multi-set flagged call: every set's job carries the flag
  flagged.add(id).add(id + 1);
  ps.push(pool.verifySignatureSets([set(id++), set(id++)], {validatePubkeys: true, batchable: true}));
  assert.deepStrictEqual(await Promise.all(ps), Array(ps.length).fill(true));
  assert.strictEqual(addon.jobs.length, id);
  const seen = new Set();
  for (const j of addon.jobs) {
    assert.ok(!seen.has(j.id), "set " + j.id + " sent twice");
    seen.add(j.id);
    assert.strictEqual((j.flags & VALIDATE) !== 0, flagged.has(j.id), "set " + j.id + " flags " + j.flags);
  }
  // the two kinds did share packages (the flag is per job, not per package)
  const byPkg = new Map();
  for (const j of addon.jobs) {
    const s = byPkg.get(j.package) || new Set();
    s.add((j.flags & VALIDATE) !== 0);
    byPkg.set(j.package, s);
  }
  assert.ok(Array.from(byPkg.values()).some((s) => s.size === 2), "no package held both kinds");
  await pool.close();
});

test("a flagged job's key error rejects its own promise with the blst code name", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
  const bad = pool.verifySignatureSets([set(1, true)], {batchable: true, validatePubkeys: true});
  const sameKeyUnflagged = pool.verifySignatureSets([set(2, true)], {batchable: true});
  const good = pool.verifySignatureSets([set(3)], {batchable: true, validatePubkeys: true});
  await assert.rejects(bad, /BLST_POINT_NOT_IN_GROUP/);
  assert.strictEqual(await sameKeyUnflagged, true);
  assert.strictEqual(await good, true);
  await assert.rejects(pool.verifySignatureSets([set(4, true)], {verifyOnMainThread: true, validatePubkeys: true}),
                       /BLST_POINT_NOT_IN_GROUP/);
  await pool.close();
});

test("verifyDeposits: one addon call, booleans per deposit; absent entry point throws", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({}, {addon});
  const dep = (b) => new Uint8Array(184).fill(b);
  const domain = new Uint8Array(32).fill(3);
  assert.deepStrictEqual(await pool.verifyDeposits([dep(1), dep(0xba), dep(2)], domain), [true, false, true]);
  assert.deepStrictEqual(addon.deposits, [{n: 3, domain: "03".repeat(32)}]);
  const packed = new Uint8Array(2 * 184).fill(9);
  assert.deepStrictEqual(await pool.verifyDeposits(packed, domain), [true, true]);
  assert.deepStrictEqual(await pool.verifyDeposits([], domain), []);
  await assert.rejects(pool.verifyDeposits([new Uint8Array(183)], domain), /184/);
  delete addon.verifyDeposits;
  await assert.rejects(pool.verifyDeposits([dep(1)], domain), /does not support verifyDeposits/);
  await pool.close();
});

test("the single-thread verifier and createBlsVerifier carry validatePubkeys and verifyDeposits", async () => {
  for (const make of [
    (addon) => new V.BlsGpuSingleThreadVerifier({}, {addon}),
    (addon) => V.createBlsVerifier({blsVerifyAllMainThread: true}, {addon}),
    (addon) => V.createBlsVerifier({}, {addon}),
  ]) {
    const addon = fakeAddon();
    const v = make(addon);
    assert.strictEqual(await v.verifySignatureSets([set(1)], {batchable: true, validatePubkeys: true}), true);
    assert.strictEqual(await v.verifySignatureSets([set(2)], {batchable: true}), true);
    assert.strictEqual(await v.verifySignatureSets([set(3)]), true);
    assert.strictEqual(await v.verifySignatureSets([set(4, true)], {batchable: true}), true); // unflagged: the key is trusted
    await assert.rejects(v.verifySignatureSets([set(5, true)], {batchable: true, validatePubkeys: true}), /BLST_POINT_NOT_IN_GROUP/);
    const flags = new Map(addon.jobs.map((j) => [j.id, (j.flags & VALIDATE) !== 0]));
    assert.deepStrictEqual([1, 2, 3, 4, 5].map((id) => flags.get(id)), [true, false, false, false, true]);
    const dep = (b) => new Uint8Array(184).fill(b);
    assert.deepStrictEqual(await v.verifyDeposits([dep(1), dep(0xba)], new Uint8Array(32)), [true, false]);
    await v.close();
    await assert.rejects(v.verifyDeposits([dep(1)], new Uint8Array(32)), /QUEUE_ERROR_QUEUE_ABORTED/);
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
