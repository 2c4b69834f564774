"use strict";
/**
 * The msgCacheEntries option and getMsgCacheStats of both verifiers
 * (lodestar_amd/js/blsGpuVerifier.js) on the CPU, with a fake addon that records what it is
 * given: the option reaches msgCacheSet once, when the context opens and before the
 * reservation; 0 or no option calls nothing; the stats are the addon's numbers.
 * Run: node tests/js/test_msg_cache_host.js   (driven by tests/test_msg_cache_bindings.py)
 */
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "blsGpuVerifier.js"));

const NUMBERS = {lookups: 70, hits: 50, pending: 3, inserts: 15, evictions: 4, bypassed: 1, full: 2, entries: 11, capacity: 4096};

function fakeAddon() {
  const m = {
    calls: [], // the order of open / msgCacheSet / reserve / msgCacheStats
    open: () => {
      m.calls.push(["open"]);
      return {ctx: true};
    },
    close() {},
    slots: () => 2,
    reserve(ctx, sets) {
      m.calls.push(["reserve", sets]);
    },
    verifyPacked(ctx, arena, setDesc, jobDesc) {
      const nJobs = jobDesc.length / 2;
      const startNs = Number(process.hrtime.bigint());
      const done = {status: new Uint8Array(nJobs).fill(1), errCode: new Int32Array(nJobs), batchRetries: 0,
                    batchSigsSuccess: 0, startNs, endNs: startNs + 1e6, workerId: 0};
      return new Promise((r) => setTimeout(() => r(done), 1));
    },
    msgCacheSet(ctx, rows) {
      assert.ok(ctx && ctx.ctx === true);
      m.calls.push(["msgCacheSet", rows]);
    },
    msgCacheStats(ctx) {
      assert.ok(ctx && ctx.ctx === true);
      m.calls.push(["msgCacheStats"]);
      return Object.assign({}, NUMBERS);
    },
  };
  return m;
}

const makers = [
  ["BlsGpuVerifier", (o, addon) => new V.BlsGpuVerifier(o, {addon})],
  ["BlsGpuSingleThreadVerifier", (o, addon) => new V.BlsGpuSingleThreadVerifier(o, {addon})],
];
const sig = new Uint8Array(96).fill(1);
const set = (id) => ({type: V.SignatureSetType.single, pubkey: new Uint8Array(48).fill(9), signingRoot: new Uint8Array(32).fill(id),
                      signature: sig});

const tests = [];
function test(name, fn) {
  tests.push({name, fn});
}

for (const [name, make] of makers) {
  test(name + ": msgCacheEntries reaches msgCacheSet once, at start-up", async () => {
    const addon = fakeAddon();
    const v = make({msgCacheEntries: 4096, reserveSets: 128}, addon);
    const want = [["open"], ["msgCacheSet", 4096]];
    if (name === "BlsGpuVerifier") want.push(["reserve", 128]); // the reservation sizes the cache's buffers: after it
    assert.deepStrictEqual(addon.calls, want);
    assert.strictEqual(v.msgCacheEntries, 4096);
    if (name === "BlsGpuVerifier") {
      assert.strictEqual(await v.verifySignatureSets([set(1), set(2)], {batchable: true}), true);
      assert.strictEqual(await v.verifySignatureSets([set(1)]), true);
    }
    assert.strictEqual(addon.calls.filter((c) => c[0] === "msgCacheSet").length, 1);
    await v.close();
  });

  test(name + ": no option, or 0, calls nothing", async () => {
    for (const o of [{}, {msgCacheEntries: 0}, {msgCacheEntries: null}]) {
      const addon = fakeAddon();
      const v = make(o, addon);
      assert.deepStrictEqual(addon.calls, [["open"]]);
      assert.strictEqual(v.msgCacheEntries, 0);
      await v.close();
    }
    // ... and works against an addon without the entry points, whose stats read zero
    const addon = fakeAddon();
    delete addon.msgCacheSet;
    delete addon.msgCacheStats;
    const v = make({}, addon);
    const st = v.getMsgCacheStats();
    assert.deepStrictEqual(Object.keys(st).sort(), Object.keys(NUMBERS).sort());
    assert.ok(Object.values(st).every((x) => x === 0));
    await v.close();
    assert.throws(() => make({msgCacheEntries: 64}, addon), /does not support msgCacheEntries/);
  });

  test(name + ": a bad msgCacheEntries is refused", async () => {
    for (const bad of [-1, 1.5, "many", NaN]) {
      const addon = fakeAddon();
      assert.throws(() => make({msgCacheEntries: bad}, addon), /non-negative integer/);
      assert.ok(!addon.calls.some((c) => c[0] === "msgCacheSet"));
    }
  });

  test(name + ": getMsgCacheStats returns the addon's numbers", async () => {
    const addon = fakeAddon();
    const v = make({msgCacheEntries: 4096}, addon);
    assert.deepStrictEqual(v.getMsgCacheStats(), NUMBERS);
    assert.deepStrictEqual(addon.calls[addon.calls.length - 1], ["msgCacheStats"]);
    await v.close();
    assert.throws(() => v.getMsgCacheStats());
  });
}

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
