"use strict";
/**
 * Per-key signature aggregates of BlsGpuVerifier (options.onAggregates; lodestar_amd/js/
 * blsGpuVerifier.js) on the CPU, with a fake addon that records the groups it is given and answers
 * with recognisable aggregates: how aggregateKey becomes a group id across the calls of one
 * package, which tags the handler gets and in which order, that the handler runs before the
 * package's promises settle, that no handler means no groups argument, and that a throwing
 * handler rejects nothing.
 * Run: node tests/js/test_aggregate_host.js   (driven by tests/test_aggregate_host.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const NO_GROUP = 0xffffffff;

/** verdict(k, msg0): the fake verdict of set k whose message starts with byte msg0 (0xee: forged).
 * A job is valid when all of its sets are.  agg[g] = 96 bytes of (g + 1), aggCount[g] = included sets. */
function fakeAddon() {
  const m = {
    calls: [], // per verifyPacked: {argc, groups: number[] | null, nGroups, priority}
    open: () => ({ctx: true}),
    close() {},
    slots: () => 2,
    verifyPacked(ctx, arena, setDesc, jobDesc, seed, priority, groups, nGroups) {
      const nJobs = jobDesc.length / 2;
      m.calls.push({argc: arguments.length, groups: groups ? Array.from(groups) : null, nGroups, priority});
      const status = new Uint8Array(nJobs);
      const agg = groups ? new Uint8Array(96 * nGroups) : undefined;
      const aggCount = groups ? new Uint32Array(nGroups) : undefined;
      if (groups) assert.strictEqual(groups.length, setDesc.length / 7, "one group word per set");
      let k = 0;
      for (let j = 0; j < nJobs; j++) {
        let ok = true;
        for (let q = 0; q < jobDesc[2 * j]; q++) ok = ok && arena[setDesc[7 * (k + q) + 3]] !== 0xee;
        status[j] = ok ? 1 : 0;
        for (let q = 0; q < jobDesc[2 * j]; q++, k++) {
          if (!groups || !ok || groups[k] === NO_GROUP) continue;
          assert.ok(groups[k] < nGroups, "group id below nGroups");
          aggCount[groups[k]]++;
          agg.fill(groups[k] + 1, 96 * groups[k], 96 * groups[k] + 96);
        }
      }
      const startNs = Number(process.hrtime.bigint());
      const done = {status, errCode: new Int32Array(nJobs), batchRetries: 0, batchSigsSuccess: 0, startNs,
                    endNs: startNs + 1e6, workerId: 0, agg, aggCount};
      return new Promise((r) => setTimeout(() => r(done), 1));
    },
  };
  return m;
}

const root = (id) => new Uint8Array(32).fill(id);
const sig = new Uint8Array(96).fill(1);
const pk = new Uint8Array(48).fill(9);
const keyed = (msg, key, tag) => ({type: V.SignatureSetType.single, pubkey: pk, signingRoot: root(msg), signature: sig,
                                   aggregateKey: key, aggregateTag: tag});

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

test("keys of different calls in one package share ids; tags arrive in package order", async () => {
  const addon = fakeAddon();
  const seen = [];
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5, onAggregates: (e) => seen.push(e)}, {addon});
  // five batchable calls buffered into one package: keys a, b, a, (none), b; the fourth set of
  // key a is forged
  const calls = [
    pool.verifySignatureSets([keyed(1, "a", 10)], {batchable: true}),
    pool.verifySignatureSets([keyed(2, "b", {bit: 3})], {batchable: true}),
    pool.verifySignatureSets([keyed(3, "a", 11)], {batchable: true}),
    pool.verifySignatureSets([{type: V.SignatureSetType.single, pubkey: pk, signingRoot: root(4), signature: sig}], {batchable: true}),
    pool.verifySignatureSets([keyed(5, "b", "t5")], {batchable: true}),
    pool.verifySignatureSets([keyed(0xee, "a", 12)], {batchable: true}),
    pool.verifySignatureSets([keyed(0xee, "c", 13)], {batchable: true}),
  ];
  assert.deepStrictEqual(await Promise.all(calls), [true, true, true, true, true, false, false]);
  assert.strictEqual(addon.calls.length, 1);
  assert.deepStrictEqual(addon.calls[0].groups, [0, 1, 0, NO_GROUP, 1, 0, 2]);
  assert.strictEqual(addon.calls[0].nGroups, 3);
  assert.strictEqual(seen.length, 1, "one handler call per package");
  const e = seen[0];
  assert.deepStrictEqual(e.map((x) => [x.key, x.count, x.tags]), [["a", 2, [10, 11]], ["b", 2, [{bit: 3}, "t5"]]]); // (c: count 0)
  assert.ok(e[0].signature instanceof Uint8Array && e[0].signature.length === 96);
  assert.deepStrictEqual(Array.from(e[0].signature), Array(96).fill(1));
  assert.deepStrictEqual(Array.from(e[1].signature), Array(96).fill(2));
  await pool.close();
});

test("a multi-set job is all or nothing; verifySignatureSetsSameMessage passes both fields", async () => {
  const addon = fakeAddon();
  const seen = [];
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5, onAggregates: (e) => seen.push(e)}, {addon});
  // one job of three sets with a forged one: its good sets are left out
  assert.strictEqual(await pool.verifySignatureSets([keyed(1, "k", 0), keyed(0xee, "k", 1), keyed(2, "k", 2)]), false);
  assert.deepStrictEqual(seen, []);
  assert.strictEqual(await pool.verifySignatureSets([keyed(1, "k", 0), keyed(2, "j", 1), keyed(3, "k", 2)]), true);
  assert.deepStrictEqual(seen[0].map((x) => [x.key, x.count, x.tags]), [["k", 2, [0, 2]], ["j", 1, [1]]]);
  seen.length = 0;
  const res = await pool.verifySignatureSetsSameMessage(
    [0, 1, 2].map((i) => ({publicKey: pk, signature: sig, aggregateKey: "same", aggregateTag: i})), root(7));
  assert.deepStrictEqual(res, [true, true, true]);
  assert.deepStrictEqual(seen[0].map((x) => [x.key, x.count, x.tags]), [["same", 3, [0, 1, 2]]]);
  await pool.close();
});

test("the handler runs before the package's promises settle", async () => {
  const addon = fakeAddon();
  const order = [];
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5, onAggregates: (e) => order.push("handler " + e[0].key)}, {addon});
  const a = pool.verifySignatureSets([keyed(1, "a", 0)], {batchable: true}).then(() => order.push("verdict a"));
  const b = pool.verifySignatureSets([keyed(2, "a", 1)], {batchable: true}).then(() => order.push("verdict b"));
  const c = pool.verifySignatureSets([keyed(3, "z", 2)], {verifyOnMainThread: true}).then(() => order.push("verdict c"));
  await Promise.all([a, b, c]);
  assert.strictEqual(order.length, 5); // one handler call for the priority package, one for the buffered one
  assert.ok(order.indexOf("handler z") >= 0 && order.indexOf("handler z") < order.indexOf("verdict c"));
  assert.ok(order.indexOf("handler a") >= 0 && order.indexOf("handler a") < order.indexOf("verdict a"));
  assert.ok(order.indexOf("handler a") < order.indexOf("verdict b"));
  // the priority package was grouped like any other
  const prio = addon.calls.find((x) => x.priority === true);
  assert.deepStrictEqual([prio.groups, prio.nGroups], [[0], 1]);
  await pool.close();
});

test("no handler: the keys are ignored and the addon gets no groups argument", async () => {
  const addon = fakeAddon();
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5}, {addon});
  assert.strictEqual(await pool.verifySignatureSets([keyed(1, "a", 0)], {batchable: true}), true);
  assert.strictEqual(await pool.verifySignatureSets([keyed(1, "a", 0)], {verifyOnMainThread: true}), true);
  assert.deepStrictEqual(addon.calls.map((x) => [x.argc, x.groups]), [[5, null], [6, null]]);
  await pool.close();
  // ... and with a handler, a package without a keyed set goes out the same way
  const addon2 = fakeAddon();
  const seen = [];
  const pool2 = new V.BlsGpuVerifier({bufferWaitMs: 5, onAggregates: (e) => seen.push(e)}, {addon: addon2});
  const plain = {type: V.SignatureSetType.single, pubkey: pk, signingRoot: root(1), signature: sig};
  assert.strictEqual(await pool2.verifySignatureSets([plain], {batchable: true}), true);
  assert.deepStrictEqual(addon2.calls.map((x) => [x.argc, x.groups]), [[5, null]]);
  assert.deepStrictEqual(seen, []);
  await pool2.close();
});

test("a throwing or rejecting handler does not reject anything; a key that is no string rejects its own call", async () => {
  const addon = fakeAddon();
  const logged = [];
  let n = 0;
  const handler = () => {
    if (n++ === 0) throw Error("pool exploded");
    return Promise.reject(Error("pool exploded later"));
  };
  const pool = new V.BlsGpuVerifier({bufferWaitMs: 5, onAggregates: handler}, {addon, logger: {error: (m) => logged.push(m)}});
  assert.strictEqual(await pool.verifySignatureSets([keyed(1, "a", 0)], {batchable: true}), true);
  assert.strictEqual(await pool.verifySignatureSets([keyed(2, "a", 0)]), true);
  await new Promise((r) => setTimeout(r, 5));
  assert.strictEqual(n, 2);
  assert.strictEqual(logged.length, 2);
  const bad = pool.verifySignatureSets([keyed(3, 17, 0)], {batchable: true});
  const good = pool.verifySignatureSets([keyed(4, "a", 1)], {batchable: true});
  await assert.rejects(bad, /aggregateKey must be a string/);
  assert.strictEqual(await good, true);
  await pool.close();
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
