"use strict";
/**
 * BlsGpuVerifier -- IBlsVerifier on one MI355X (gfx950), a drop-in for Lodestar's
 * BlsMultiThreadWorkerPool (/root/reference/packages/beacon-node/src/chain/bls/multithread/
 * index.ts) and BlsSingleThreadVerifier (chain/bls/singleThread.ts:14-35).
 *
 * What is kept from the reference, name for name (the file:line is the reference code each
 * method restates):
 *   verifySignatureSets   index.ts:151-191  verifyOnMainThread shortcut, chunks of <= 128
 *                         sets, AND over the chunks, empty chunk list -> throw
 *   canAcceptWork         index.ts:143-149  back-pressure, on sets for a GPU: queued +
 *                         buffered + in-flight sets < maxPendingSigs
 *   close                 index.ts:193-217  pending jobs reject with QueueError
 *                         QUEUE_ERROR_QUEUE_ABORTED
 *   _queueBlsWork         index.ts:255-302  batchable jobs buffered until > 32 sigs or
 *                         100 ms; others queued and run on the next macrotask
 *   _runJob/_prepareWork  index.ts:307-420  packages sized for the GPU (class comment);
 *                         per-job resolve/reject; metrics
 *   _runBufferedJobs      index.ts:425-431
 *   chunkifyMaximizeChunkSize  multithread/utils.ts:4-19
 * What replaces the worker threads and @chainsafe/blst: the N-API addon
 * (lodestar_amd/napi/lsg_napi.c) over the C ABI (include/lodestar_bls.h).  A package is
 * packed into one byte arena (packJobs) and handed to addon.verifyPacked, whose native
 * package thread submits and waits (neither the JS thread nor libuv's pool blocks); the
 * promise settles with per-job verdict arrays.  The GPU applies the worker's batch + per-job
 * retry rules (worker.ts:30-106) itself, so one package costs one round trip.  Aggregate sets
 * send all their pubkeys; the GPU sums them (utils.ts:11).
 *
 * Node-wide: chain.ts:195-198 builds ONE verifier per node, its pool spanning every core
 * (multithread/poolSize.ts:7).  options.devices = [0, 1, ...] opens one context over all the
 * node's GPUs (lsg_init_devices): a package is split into whole jobs per GPU, the GPUs'
 * partials are all-gathered over RCCL and checked by one final exponentiation (SURVEY 8e).
 *
 * BlsGpuSingleThreadVerifier restates BlsSingleThreadVerifier (singleThread.ts:14-35): one
 * synchronous maybeBatch call per verifySignatureSets, no queue, no retry, opts ignored.
 * createBlsVerifier picks between the two as chain.ts:196-198 does (blsVerifyAllMainThread).
 *
 * Metrics: the reference's names and observation points (metrics/metrics/lodestar.ts:350-430,
 * multithread/index.ts:135-140,319-381): queueLength, workersBusy (collected at scrape time),
 * jobWaitTime, totalJobsGroupsStarted, totalJobsStarted,
 * totalSigSetsStarted, timePerSigSet, jobsWorkerTime{workerId}, latencyToWorker,
 * latencyFromWorker, successJobsSignatureSetsCount, errorJobsSignatureSetsCount,
 * batchRetries, batchSigsSuccess, mainThreadDurationInThreadPool, bls.aggregatedPubkeys.
 * "Worker" times are the GPU package's start/end (lsg_stats, CLOCK_MONOTONIC = the clock of
 * process.hrtime.bigint()); workerId is the pipeline slot that ran the package.
 *
 * Extensions required by the north star (SURVEY.md 8b, not in the reference snapshot):
 *   opts.priority                  queue at the head instead of the tail
 *   verifySignatureSetsSameMessage per-set verdicts for sets sharing one message
 * Objects that carry their own, untrusted keys (INTEGRATION.md):
 *   opts.validatePubkeys           PublicKey.fromBytes(pk, affine, true) for the call's keys, on
 *                                  the GPU inside the package (signatureSets/blsToExecutionChange.ts:32)
 *   verifyDeposits                 block/processDeposit.ts:47-66 for a list of DepositData
 * Op pools (INTEGRATION.md "Op pools", SURVEY.md 8f(7)):
 *   options.onAggregates           per package and aggregateKey, the sum of the verified sets'
 *                                  signatures (set.aggregateKey, set.aggregateTag)
 */

const MAX_SIGNATURE_SETS_PER_JOB = 128;
const MAX_BUFFERED_SIGS = 32;
const MAX_BUFFER_WAIT_MS = 100;
const MAX_JOBS_CAN_ACCEPT_WORK = 512;

const JOB_BATCHABLE = 1;
const JOB_PRIORITY = 2;
const JOB_VALIDATE_KEYS = 4; // LSG_JOB_VALIDATE_KEYS: KeyValidate of the job's byte keys on the GPU

const LSG_INVALID = 0;
const LSG_VALID = 1;
const LSG_ERROR = 2;

/** blst error names (blst.h BLST_ERROR) + @chainsafe/blst's size error */
const BLST_NAMES = {
  0: "BLST_SUCCESS",
  1: "BLST_BAD_ENCODING",
  2: "BLST_POINT_NOT_ON_CURVE",
  3: "BLST_POINT_NOT_IN_GROUP",
  4: "BLST_AGGR_TYPE_MISMATCH",
  5: "BLST_VERIFY_FAIL",
  6: "BLST_PK_IS_INFINITY",
  7: "BLST_BAD_SCALAR",
  10: "BLST_INVALID_SIZE",
};

/** Error text for a job error code, in the form the reference's callers match on: the BLST
 * code name is a substring (multithread.test.ts:97 "BLST_INVALID_SIZE"). */
function errorMessage(code) {
  if (code === 100) return "Empty signature set"; // maybeBatch.ts:29-31
  if (code === 101) return "EMPTY_AGGREGATE_ARRAY"; // PublicKey.aggregate([])
  if (code === 103) return "Unknown committee or bit length mismatch"; // LSG_ERR_BAD_COMMITTEE
  return "BLST_ERROR: " + (BLST_NAMES[code] || "BLST_UNKNOWN_" + code);
}

/** util/queue/errors.ts:3-16 */
const QueueErrorCode = {
  QUEUE_ABORTED: "QUEUE_ERROR_QUEUE_ABORTED",
  QUEUE_MAX_LENGTH: "QUEUE_ERROR_QUEUE_MAX_LENGTH",
};

class QueueError extends Error {
  constructor(type) {
    super(type.code);
    this.type = type;
    this.code = type.code;
  }
}

/** state-transition/src/util/signatureSets.ts:5-8 */
const SignatureSetType = {single: "single", aggregate: "aggregate"};

/**
 * Splits an array into an array of arrays maximizing the size of the smallest chunk
 * (multithread/utils.ts:4-19).
 */
function chunkifyMaximizeChunkSize(arr, minPerChunk) {
  const chunkCount = Math.floor(arr.length / minPerChunk);
  if (chunkCount <= 1) {
    return [arr];
  }
  const perChunk = Math.ceil(arr.length / chunkCount);
  const arrArr = [];
  for (let i = 0; i < arr.length; i += perChunk) {
    arrArr.push(arr.slice(i, i + perChunk));
  }
  return arrArr;
}

/** PublicKey -> bytes.  Accepts raw Uint8Arrays (96 B uncompressed / 48 B compressed) or
 * @chainsafe/bls PublicKey objects (toBytes(format)). */
function pubkeyBytes(pk) {
  if (pk instanceof Uint8Array) return pk;
  if (pk && typeof pk.toBytes === "function") return pk.toBytes("uncompressed");
  throw Error("Unknown public key type");
}

/** ISignatureSet -> the addon's set (utils.ts:5-17 getAggregatedPubkey, with the sum done on
 * the GPU instead of the main thread). */
function serializeSet(set) {
  if (set.signingObject !== undefined) {
    checkMsgObject(set);
    const message = new Uint8Array(set.signingObject.length + 32);
    message.set(set.signingObject, 0);
    message.set(set.domain, set.signingObject.length);
    const kind = msgObjectKind(set);
    const out = {...serializeSet({...set, signingObject: undefined, signingObjectKind: undefined, signingRoot: message}), messageObject: true};
    if (kind !== 0) out.messageKind = kind;
    return out;
  }
  // signers named by a committee loaded with loadCommittees() plus participation bits (8f(5))
  if (set.committee !== undefined) {
    checkBitsSet(set);
    return {committee: set.committee, bits: set.bits, bitLen: set.bitLen, message: set.signingRoot, signature: set.signature};
  }
  // ... or by a list of committees plus one bitfield over their concatenation (an Electra aggregate)
  if (set.committees !== undefined) {
    checkBitsMultiSet(set);
    return {committees: set.committees, bits: set.bits, bitLen: set.bitLen, message: set.signingRoot, signature: set.signature};
  }
  // signers named by validator index into the device pubkey table (SURVEY 8f(1)):
  // loadPubkeys() mirrors index2pubkey; the set carries its attesting indices
  if (set.pubkeyIndices !== undefined) {
    const ix = set.pubkeyIndices instanceof Uint32Array ? set.pubkeyIndices : Uint32Array.from(set.pubkeyIndices);
    return {pubkeyIndices: ix, message: set.signingRoot, signature: set.signature};
  }
  let pubkeys;
  switch (set.type) {
    case SignatureSetType.single:
      pubkeys = [pubkeyBytes(set.pubkey)];
      break;
    case SignatureSetType.aggregate:
      pubkeys = set.pubkeys.map(pubkeyBytes);
      break;
    default:
      throw Error("Unknown signature set type");
  }
  return {pubkeys, message: set.signingRoot, signature: set.signature};
}

/**
 * Every call's promise is made with this one executor, which hands the resolve function out
 * through a module variable: no closure per call.  A job keeps only that function in its page
 * (the reject function dies young) and is settled by calling it with its boolean verdict, or
 * with a rejected promise for an error -- one promise and one reaction job per call.  What
 * bounds the JS thread is the young-generation collector: node 12's nursery is 16 MB whatever
 * --max-semi-space-size says, so at ~1M calls per 100 ms every pending call survives several
 * scavenges and is copied twice; each retained object per call costs.  Measured in node 12
 * with a 5-package pipeline (tools/node_host_ceiling.js, profiles/r06_node_host_ceiling.txt):
 * `shared.then(pick[i])` (rounds 3-5: a second promise, a reaction and a second microtask per
 * call) 1.3 us per call, resolve + reject kept 0.95 us, resolve only 0.75 us.
 */
let RES = null;
function EXEC(resolve) {
  RES = resolve;
}

/**
 * verifySignatureSetsMaybeBatch(sets) (maybeBatch.ts:16-39) as ONE non-batchable job sent
 * straight to the addon, outside the queue and ahead of it: verifyPacked's priority flag runs it
 * on the addon's priority thread (never behind the package threads' queue) and on the
 * library's high-priority streams.  The reference runs this path synchronously on the main
 * thread (multithread/index.ts:155-168, ~0.9 ms of blst); here the caller's promise settles
 * with the verdict and the JS thread keeps running meanwhile.  No retry: one job is one
 * maybeBatch call; an error rejects with its BLST code (e.g. BLST_INVALID_SIZE).
 */
function verifyDirect(addon, ctx, sets, seed, validate = false, onAggregates = null, logger = null) {
  const page = new JobPage(false, true, null, validate);
  const p = page.push(sets);
  const pkg = packJobs([page, 0, 1], sets.length, undefined, 0, onAggregates !== null);
  if (pkg.nJobs === 1) {
    const call =
      pkg.groups === null
        ? addon.verifyPacked(ctx, pkg.arena, pkg.setDesc, pkg.jobDesc, seed, true)
        : addon.verifyPacked(ctx, pkg.arena, pkg.setDesc, pkg.jobDesc, seed, true, pkg.groups, pkg.groupKeys.length);
    call.then(
      (r) => {
        if (pkg.groups !== null) deliverAggregates(pkg, r, onAggregates, logger);
        settleJobs(pkg.ranges, r.status, r.errCode);
      },
      (e) => page.fail(0, e)
    );
  }
  return p;
}

/** Limits of lsg_committees_set (include/lodestar_bls.h) */
const MAX_COMMITTEE_ID = 1 << 20;
const MAX_COMMITTEE_LEN = 131072;
const PK_BITS = 8; // LSG_PK_BITS
const PK_BITS_MULTI = 12; // LSG_PK_BITS_MULTI
const MAX_SET_COMMITTEES = 64; // LSG_MAX_SET_COMMITTEES
const NO_GROUP = 0xffffffff; // LSG_NO_GROUP

/** A set that names its signers as {committee, bits, bitLen}: committee is an id given to
 * loadCommittees, bits the participation bitfield in SSZ order without a delimiter bit (member k
 * is bit k & 7 of byte k >> 3, e.g. a BitArray's uint8Array), bitLen the committee's length. */
function checkBitsSet(set) {
  if (!Number.isInteger(set.committee) || set.committee < 0 || set.committee >= MAX_COMMITTEE_ID) {
    throw Error("committee must be an id below 2^20");
  }
  if (!Number.isInteger(set.bitLen) || set.bitLen < 0 || set.bitLen > MAX_COMMITTEE_LEN) {
    throw Error("bitLen must be the committee's length");
  }
  if (!(set.bits instanceof Uint8Array) || set.bits.length < ((set.bitLen + 7) >> 3)) {
    throw Error("bits must be a Uint8Array of at least ceil(bitLen / 8) bytes");
  }
}

/** A set that names its signers as {committees, bits, bitLen} (EIP-7549: an aggregate spanning
 * committees): committees lists ids given to loadCommittees -- at most 64, in the order their
 * members appear in the bitfield; they may repeat -- bits is one participation bitfield over the
 * concatenation of the listed committees (SSZ order, no delimiter bit), bitLen the sum of their
 * lengths. */
function checkBitsMultiSet(set) {
  const ids = set.committees;
  if (!(ids instanceof Uint32Array) && !Array.isArray(ids)) throw Error("committees must be an array of committee ids");
  if (ids.length > MAX_SET_COMMITTEES) throw Error("a set lists at most 64 committees");
  for (let c = 0; c < ids.length; c++) {
    if (!Number.isInteger(ids[c]) || ids[c] < 0 || ids[c] >= MAX_COMMITTEE_ID) throw Error("committee must be an id below 2^20");
  }
  if (!Number.isInteger(set.bitLen) || set.bitLen < 0 || set.bitLen > MAX_SET_COMMITTEES * MAX_COMMITTEE_LEN) {
    throw Error("bitLen must be the sum of the committees' lengths");
  }
  if (!(set.bits instanceof Uint8Array) || set.bits.length < ((set.bitLen + 7) >> 3)) {
    throw Error("bits must be a Uint8Array of at least ceil(bitLen / 8) bytes");
  }
}

/** participants of a {committee, bits, bitLen} set: the set bits among the first bitLen */
function countBits(bits, bitLen) {
  let n = 0;
  const full = bitLen >> 3;
  for (let i = 0; i <= full && i < bits.length; i++) {
    let b = i < full ? bits[i] : bits[i] & ((1 << (bitLen & 7)) - 1);
    for (; b; b &= b - 1) n++;
  }
  return n;
}

/** loadCommittees' arguments -> (indices, offsets) of lsg_committees_set */
function flattenCommittees(firstId, committees) {
  if (!Number.isInteger(firstId) || firstId < 0 || !Array.isArray(committees) || firstId + committees.length > MAX_COMMITTEE_ID) {
    throw Error("loadCommittees(firstId, committees): ids must stay below 2^20");
  }
  const offsets = new Uint32Array(committees.length + 1);
  for (let c = 0; c < committees.length; c++) {
    const m = committees[c];
    if (!(m instanceof Uint32Array) && !Array.isArray(m)) throw Error("a committee must be an array of validator indices");
    if (m.length > MAX_COMMITTEE_LEN) throw Error("a committee has at most 131072 members");
    offsets[c + 1] = offsets[c] + m.length;
  }
  const indices = new Uint32Array(offsets[committees.length]);
  for (let c = 0; c < committees.length; c++) {
    const m = committees[c];
    for (let k = 0; k < m.length; k++) {
      if (!Number.isInteger(m[k]) || m[k] < 0 || m[k] > 0xffffffff) throw Error("a committee member must be a validator index");
      indices[offsets[c] + k] = m[k];
    }
  }
  return {indices, offsets};
}

function loadCommitteesSync(addon, ctx, firstId, committees) {
  const {indices, offsets} = flattenCommittees(firstId, committees);
  if (typeof addon.committeesSet !== "function") throw Error("the addon does not support loadCommittees");
  return Array.from(addon.committeesSet(ctx, firstId, indices, offsets));
}

/** options.msgCacheEntries rows of hashed messages H(m) per device, kept across packages
 * (lsg_msg_cache_set; INTEGRATION.md "Message cache"), set once when the context opens; 0 or
 * absent: the library is not called at all.  Returns the rows in effect. */
function msgCacheOpen(addon, ctx, entries) {
  const rows = entries === undefined || entries === null ? 0 : Number(entries);
  if (!Number.isInteger(rows) || rows < 0) throw Error("msgCacheEntries must be a non-negative integer");
  if (rows === 0) return 0;
  if (typeof addon.msgCacheSet !== "function") throw Error("the addon does not support msgCacheEntries");
  addon.msgCacheSet(ctx, rows);
  return rows;
}

const MSG_CACHE_COUNTERS = ["lookups", "hits", "pending", "inserts", "evictions", "bypassed", "full", "entries", "capacity"];

function msgCacheStatsSync(addon, ctx) {
  if (typeof addon.msgCacheStats === "function") return addon.msgCacheStats(ctx);
  return Object.fromEntries(MSG_CACHE_COUNTERS.map((k) => [k, 0]));
}

/** utils.ts:19-26 */
function getAggregatedPubkeysCount(sets) {
  let n = 0;
  for (const set of sets) {
    if (set.committee !== undefined || set.committees !== undefined) n += set.bits instanceof Uint8Array ? countBits(set.bits, set.bitLen) : 0;
    else if (set.pubkeyIndices !== undefined) n += set.pubkeyIndices.length;
    else if (set.type === SignatureSetType.aggregate) n += set.pubkeys.length;
  }
  return n;
}

/**
 * block/processDeposit.ts:47-66 for a list of deposits in one device pass (lsg_verify_deposits):
 * KeyValidate of the deposit's own key, Signature.fromBytes(sig, affine, true) and the verify
 * over computeSigningRoot(DepositMessage, domain).  depositDatas: SSZ-serialized DepositData,
 * 184 bytes each (pubkey 48, withdrawalCredentials 32, amount u64 LE, signature 96), as a list
 * of Uint8Arrays or one concatenated Uint8Array.  Returns one boolean per deposit: true exactly
 * when processDeposit would go on to add the validator (a bad key or signature is false, never
 * an error: the reference skips such a deposit).  The addon call is synchronous: the JS thread
 * is blocked until the verdicts are back (~20 ms for 16,384 deposits, ~9 ms for a handful),
 * as processDeposit's own blst calls block it in the reference; while the verifier's packages
 * hold every pipeline slot the addon waits for one instead of failing.
 */
function verifyDepositsSync(addon, ctx, depositDatas, domain) {
  let data = depositDatas;
  if (!(data instanceof Uint8Array)) {
    data = new Uint8Array(184 * depositDatas.length);
    for (let i = 0; i < depositDatas.length; i++) {
      if (!(depositDatas[i] instanceof Uint8Array) || depositDatas[i].length !== 184) throw Error("DepositData must be 184 serialized bytes");
      data.set(depositDatas[i], 184 * i);
    }
  }
  if (data.length % 184 !== 0) throw Error("DepositData must be 184 serialized bytes");
  if (typeof addon.verifyDeposits !== "function") throw Error("the addon does not support verifyDeposits");
  const r = addon.verifyDeposits(ctx, data, domain);
  const out = new Array(r.valid.length);
  for (let i = 0; i < out.length; i++) out[i] = r.valid[i] === 1;
  return out;
}

function loadAddon() {
  // eslint-disable-next-line global-require
  return require("../napi/lsg_napi.node");
}

/** A set may give its message as the SSZ serialization of the signed object plus its domain
 * ({signingObject, domain} instead of signingRoot; LSG_MSG_OBJECT, SURVEY.md 8f(6)): the
 * signing root is computed on the GPU as the package's first stage.  The object's length
 * selects its kind: uint64, two uint64 fields, Root, BLSToExecutionChange, DepositMessage,
 * BeaconBlockHeader, AttestationData, ContributionAndProof.  A variable-size object names its
 * kind beside it (signingObjectKind: "AggregateAndProof" | "AggregateAndProofElectra"): the kind
 * tag travels in bits 24..30 of the length word (LSG_MSG_KIND_*), and the object's structure --
 * both offsets, the bitlist's delimiter bit and limit, the length -- is checked here, at call
 * time, as the library checks it at its entry points. */
const MSG_OBJECT = 0x80000000; // LSG_MSG_OBJECT
const MSG_KIND_SHIFT = 24; // LSG_MSG_KIND_SHIFT
const MSG_OBJECT_LENGTHS = [8, 16, 32, 76, 88, 112, 128, 264];
// signingObjectKind -> {tag, where the bitlist starts, its limit in bits}
const MSG_OBJECT_KINDS = {
  AggregateAndProof: {tag: 1, bitsOff: 336, maxBits: 2048},
  AggregateAndProofElectra: {tag: 2, bitsOff: 344, maxBits: 131072},
};
function msgObjectKind(set) {
  return set.signingObjectKind === undefined ? 0 : MSG_OBJECT_KINDS[set.signingObjectKind].tag;
}
function checkMsgObject(set) {
  const obj = set.signingObject;
  if (set.signingObjectKind !== undefined) {
    const kind = Object.prototype.hasOwnProperty.call(MSG_OBJECT_KINDS, set.signingObjectKind) ? MSG_OBJECT_KINDS[set.signingObjectKind] : null;
    if (kind === null) throw Error(`signingObjectKind must be one of ${Object.keys(MSG_OBJECT_KINDS).join(", ")}`);
    const {bitsOff, maxBits} = kind;
    if (!(obj instanceof Uint8Array) || obj.length <= bitsOff || obj.length > bitsOff + maxBits / 8 + 1) {
      throw Error(`signingObject of kind ${set.signingObjectKind} must be a Uint8Array of ${bitsOff + 1} to ${bitsOff + maxBits / 8 + 1} bytes`);
    }
    const u32 = (at) => (obj[at] | (obj[at + 1] << 8) | (obj[at + 2] << 16) | (obj[at + 3] << 24)) >>> 0;
    if (u32(8) !== 108 || u32(108) !== bitsOff - 108) throw Error(`signingObject is not a serialized ${set.signingObjectKind}: offsets`);
    const last = obj[obj.length - 1];
    if (last === 0) throw Error("signingObject's aggregation bits have no delimiter bit");
    if (8 * (obj.length - bitsOff - 1) + (31 - Math.clz32(last)) > maxBits) throw Error(`signingObject's aggregation bits exceed ${maxBits}`);
  } else if (!(obj instanceof Uint8Array) || !MSG_OBJECT_LENGTHS.includes(obj.length)) {
    throw Error(`signingObject must be a Uint8Array of ${MSG_OBJECT_LENGTHS.join(", ")} bytes`);
  }
  if (!(set.domain instanceof Uint8Array) || set.domain.length !== 32) {
    throw Error("domain must be a Uint8Array of 32 bytes");
  }
}

/** Reference set shape check done at call time, as serializeSet throws there (index.ts:177). */
function checkSet(set) {
  if (set.signingObject !== undefined) checkMsgObject(set);
  if (set.committee !== undefined) {
    checkBitsSet(set);
    return;
  }
  if (set.committees !== undefined) {
    checkBitsMultiSet(set);
    return;
  }
  if (set.pubkeyIndices === undefined && set.type !== SignatureSetType.single && set.type !== SignatureSetType.aggregate) {
    throw Error("Unknown signature set type");
  }
}

/** FIFO with O(1) shift (Array.prototype.shift is O(n) on long queues). */
class Fifo {
  constructor() {
    this.items = [];
    this.head = 0;
  }
  get length() {
    return this.items.length - this.head;
  }
  peek() {
    return this.head < this.items.length ? this.items[this.head] : undefined;
  }
  push(x) {
    this.items.push(x);
  }
  shift() {
    if (this.head >= this.items.length) return undefined;
    const x = this.items[this.head];
    this.items[this.head++] = undefined;
    if (this.head > 1024 && this.head * 2 > this.items.length) {
      this.items = this.items.slice(this.head);
      this.head = 0;
    }
    return x;
  }
  drain() {
    const out = this.items.slice(this.head);
    this.items = [];
    this.head = 0;
    return out;
  }
}

/**
 * Jobs live in pages: parallel arrays (a job's sets, its resolve and reject functions), no
 * object per job.  A page is the reference's buffer of batchable jobs (index.ts:255-302) or a
 * run of non-batchable jobs queued one after another, and it keeps accepting jobs while it
 * waits at the tail of the queue: a batchable job that arrives after its buffer was flushed to
 * the queue joins it there instead of opening a new buffer (it becomes eligible sooner, never
 * later, than in the reference; verdicts do not depend on it).  A package takes jobs from the
 * head page onwards one job at a time, as prepareWork does (index.ts:400-418), so a page can
 * be spread over several packages; a page a package has taken from accepts no more jobs.
 * The job flags are the page's: a page holds jobs of one kind only (batchable, priority,
 * validate), so calls with and without opts.validatePubkeys never share a page -- they may
 * share a package, where each job carries its own page's flag word.  One effect on timing: a
 * batchable call of the other kind sends the open buffer to the queue before its 100 ms or
 * 32-sig limit, so under alternating flagged and unflagged traffic unflagged jobs reach the
 * queue earlier and in smaller pages than they would alone (later calls of that kind rejoin
 * the queued tail page while it is open).  Verdicts do not depend on it.
 */
const PAGE_JOBS = 8192;

class JobPage {
  /** @param {number[]|null} added  per-job Date.now() at queueing (jobWaitTime metric) */
  constructor(batchable, priority, added, validate = false) {
    this.batchable = batchable;
    this.priority = priority;
    this.validate = validate; // opts.validatePubkeys: its jobs carry JOB_VALIDATE_KEYS
    this.sets = []; // per job: its sets (dropped once packed)
    this.res = []; // per job: its promise's resolve function (undefined once settled)
    this.added = added;
    this.n = 0; // jobs
    this.nSigs = 0;
    this.multi = false; // some job does not hold exactly one set
    this.taken = 0; // jobs [0, taken) are in packages (or settled)
    this.open = true; // accepts jobs
    this.firstPush = 0; // buffered pages: Date.now() of the first job
  }
  push(sets) {
    const p = new Promise(EXEC);
    this.sets.push(sets);
    this.res.push(RES);
    if (this.added) this.added.push(Date.now());
    this.n++;
    this.nSigs += sets.length;
    if (sets.length !== 1) this.multi = true;
    if (this.n >= PAGE_JOBS) this.open = false;
    return p;
  }
  fail(j, error) {
    const r = this.res[j];
    if (r === undefined) return;
    this.res[j] = undefined;
    this.sets[j] = undefined;
    r(Promise.reject(error));
  }
  /** rejects every job not yet in a package */
  failRest(error) {
    for (let j = this.taken; j < this.n; j++) this.fail(j, error);
    this.taken = this.n;
    this.open = false;
  }
}

/** Settles the jobs of a package's ranges ([page, start, end] triples) with the addon's
 * per-job results, in packing order; jobs settled while packing (unserialisable sets) were
 * left out of the package and are skipped here. */
function settleJobs(ranges, status, codes) {
  let i = 0;
  for (let r = 0; r < ranges.length; r += 3) {
    const page = ranges[r];
    const res = page.res;
    for (let j = ranges[r + 1], end = ranges[r + 2]; j < end; j++) {
      const f = res[j];
      if (f === undefined) continue;
      const st = status[i];
      const code = codes[i];
      i++;
      res[j] = undefined;
      if (st === LSG_VALID) f(true);
      else if (st === LSG_INVALID) f(false);
      else f(Promise.reject(Error(errorMessage(code))));
    }
  }
}

/** Rejects every still-pending job of a package's ranges (the addon's call failed). */
function failJobs(ranges, error) {
  for (let r = 0; r < ranges.length; r += 3) {
    const page = ranges[r];
    for (let j = ranges[r + 1], end = ranges[r + 2]; j < end; j++) page.fail(j, error);
  }
}

const SET_DESC_WORDS = 7; // pkOff, pkLen, nPks, msgOff, msgLen, sigOff, sigLen (lsg_napi.c verifyPacked)

/**
 * A package's jobs in the addon's packed form: one byte arena with every key, message and
 * signature, 7 descriptor words per set and 2 per job -- the role of the structured clone of
 * BlsWorkReq[] in multithread/index.ts:335 (and of getAggregatedPubkey + toBytes,
 * index.ts:177, except that aggregate keys are summed on the GPU).  `ranges` are
 * [page, start, end] triples.  A job whose sets cannot be serialized is rejected on its own
 * and left out.  `into` (optional) is a previous package's buffers, reused when large enough
 * (fresh multi-MB typed arrays per package cost GC time).  Packed jobs drop their sets.
 */
function packJobs(ranges, nSigs, into, minSigs = 0, grouped = false) {
  // grouped (the verifier has an onAggregates handler): a set's aggregateKey becomes its group
  // id -- one id per distinct key of the package, whichever call the set came from -- and its
  // aggregateTag is kept for the handler.  A package without a keyed set has groups === null.
  let groups = null;
  let groupIds = null; // key -> id
  let groupKeys = null; // id -> key
  let groupTags = null; // per set
  const groupOf = (set, k) => {
    const key = set.aggregateKey;
    if (key === undefined) {
      if (groups !== null) groups[k] = NO_GROUP;
      return;
    }
    if (typeof key !== "string") throw Error("aggregateKey must be a string");
    if (groups === null) {
      const len = Math.max(nSigs, minSigs);
      groups = into && into.groupsBuf && into.groupsBuf.length >= len ? into.groupsBuf : new Uint32Array(len);
      groups.fill(NO_GROUP);
      groupIds = new Map();
      groupKeys = [];
      groupTags = [];
    }
    let id = groupIds.get(key);
    if (id === undefined) {
      id = groupKeys.length;
      groupIds.set(key, id);
      groupKeys.push(key);
    }
    groups[k] = id;
    groupTags[k] = set.aggregateTag;
  };
  // 224 bytes per set: one raw key, a 32-byte root, a signature.  Sets that carry more (aggregate
  // keys, signingObject + domain: up to 16,761 message bytes) grow the arena in put(); the grown
  // buffer comes back as arenaBuf, so a verifier's later packages of that kind reuse it
  let cap = Math.max(nSigs, minSigs) * 224 + 256;
  let arena = into && into.arenaBuf.length >= cap ? into.arenaBuf : new Uint8Array(cap);
  cap = arena.length;
  let off = 0;
  const put = (bytes) => {
    const n = bytes.length;
    if (off + n > cap) {
      while (off + n > cap) cap *= 2;
      const grown = new Uint8Array(cap);
      grown.set(arena.subarray(0, off));
      arena = grown;
    }
    const o = off;
    arena.set(bytes, o);
    off += n;
    return o;
  };
  const setDescBuf =
    into && into.setDescBuf.length >= SET_DESC_WORDS * nSigs ? into.setDescBuf : new Uint32Array(SET_DESC_WORDS * Math.max(nSigs, minSigs));
  let nJobs = 0;
  for (let r = 0; r < ranges.length; r += 3) nJobs += ranges[r + 2] - ranges[r + 1];
  const jobDescBuf = into && into.jobDescBuf.length >= 2 * nJobs ? into.jobDescBuf : new Uint32Array(2 * Math.max(nJobs, minSigs));
  const sd = setDescBuf;
  let k = 0;
  let j = 0;
  for (let r = 0; r < ranges.length; r += 3) {
    const page = ranges[r];
    const flags = (page.batchable ? JOB_BATCHABLE : 0) | (page.priority ? JOB_PRIORITY : 0) | (page.validate ? JOB_VALIDATE_KEYS : 0);
    const pageSets = page.sets;
    for (let q = ranges[r + 1], qEnd = ranges[r + 2]; q < qEnd; q++) {
      const sets = pageSets[q];
      if (page.res[q] === undefined) continue; // already settled (close)
      pageSets[q] = undefined;
      const off0 = off;
      const k0 = k;
      try {
        for (let si = 0; si < sets.length; si++) {
          const set = sets[si];
          const d = SET_DESC_WORDS * k;
          const pk1 =
            set.committee === undefined && set.committees === undefined && set.pubkeyIndices === undefined && set.type === SignatureSetType.single
              ? set.pubkey
              : null;
          // the message: the signing root, or the signed object followed by its domain
          const dom = set.signingObject === undefined ? null : set.domain;
          if (dom !== null) checkMsgObject(set);
          const root = dom === null ? set.signingRoot : set.signingObject;
          const msgWord = dom === null ? root.length : MSG_OBJECT + msgObjectKind(set) * (1 << MSG_KIND_SHIFT) + root.length + 32;
          const sig = set.signature;
          const msgBytes = dom === null ? root.length : root.length + 32;
          if (grouped) groupOf(set, k);
          if (pk1 instanceof Uint8Array && pk1.length !== PK_BITS && pk1.length !== PK_BITS_MULTI && off + pk1.length + msgBytes + sig.length <= cap) {
            // the common shape (one raw key): three copies, no helper calls
            arena.set(pk1, off);
            sd[d] = off;
            sd[d + 1] = pk1.length;
            sd[d + 2] = 1;
            off += pk1.length;
            arena.set(root, off);
            sd[d + 3] = off;
            sd[d + 4] = msgWord;
            off += root.length;
            if (dom !== null) {
              arena.set(dom, off);
              off += 32;
            }
            arena.set(sig, off);
            sd[d + 5] = off;
            sd[d + 6] = sig.length;
            off += sig.length;
            k++;
            continue;
          }
          if (set.committee !== undefined) {
            // committee id (host byte order), then the first ceil(bitLen / 8) bytes of the bitfield
            checkBitsSet(set);
            const id = new Uint32Array([set.committee]);
            sd[d] = put(new Uint8Array(id.buffer));
            put(set.bits.subarray(0, (set.bitLen + 7) >> 3));
            sd[d + 1] = PK_BITS;
            sd[d + 2] = set.bitLen;
          } else if (set.committees !== undefined) {
            // the count, the committee ids (host byte order), then the first ceil(bitLen / 8) bytes
            checkBitsMultiSet(set);
            const head = new Uint32Array(1 + set.committees.length);
            head[0] = set.committees.length;
            head.set(set.committees, 1);
            sd[d] = put(new Uint8Array(head.buffer));
            put(set.bits.subarray(0, (set.bitLen + 7) >> 3));
            sd[d + 1] = PK_BITS_MULTI;
            sd[d + 2] = set.bitLen;
          } else if (set.pubkeyIndices !== undefined) {
            const ix = set.pubkeyIndices instanceof Uint32Array ? set.pubkeyIndices : Uint32Array.from(set.pubkeyIndices);
            sd[d] = put(new Uint8Array(ix.buffer, ix.byteOffset, 4 * ix.length));
            sd[d + 1] = 4; // LSG_PK_INDEX
            sd[d + 2] = ix.length;
          } else if (set.type === SignatureSetType.single) {
            const pk = pubkeyBytes(set.pubkey);
            sd[d] = put(pk);
            // (8 or 12 bytes: an unknown key length, not LSG_PK_BITS / LSG_PK_BITS_MULTI)
            sd[d + 1] = pk.length === PK_BITS || pk.length === PK_BITS_MULTI ? 0 : pk.length;
            sd[d + 2] = 1;
          } else if (set.type === SignatureSetType.aggregate) {
            const pks = set.pubkeys;
            const len = pks.length ? pubkeyBytes(pks[0]).length : 96;
            sd[d] = off;
            for (const pk of pks) {
              const b = pubkeyBytes(pk);
              if (b.length !== len) throw Error("every pubkey of an aggregate set must have the same encoding");
              put(b);
            }
            sd[d + 1] = len === PK_BITS || len === PK_BITS_MULTI ? 0 : len;
            sd[d + 2] = pks.length;
          } else {
            throw Error("Unknown signature set type");
          }
          sd[d + 3] = put(root);
          if (dom !== null) put(dom);
          sd[d + 4] = msgWord;
          sd[d + 5] = put(sig);
          sd[d + 6] = sig.length;
          k++;
        }
      } catch (e) {
        off = off0;
        k = k0;
        page.fail(q, e);
        continue;
      }
      jobDescBuf[2 * j] = sets.length;
      jobDescBuf[2 * j + 1] = flags;
      j++;
    }
  }
  return {
    ranges,
    nJobs: j,
    arena: arena.subarray(0, off),
    setDesc: sd.subarray(0, SET_DESC_WORDS * k),
    jobDesc: jobDescBuf.subarray(0, 2 * j),
    arenaBuf: arena,
    setDescBuf,
    jobDescBuf,
    nSigs: k,
    groups: groups === null ? null : groups.subarray(0, k),
    groupsBuf: groups !== null ? groups : into && into.groupsBuf ? into.groupsBuf : null,
    groupKeys,
    groupTags,
  };
}

/**
 * The onAggregates call of one grouped package (SURVEY 8f(7)): per key with at least one verified
 * signature, {key, signature: the 96-byte compressed sum the device returned, count, tags: the
 * aggregateTag of every included set in package order}; no call when no key has one.  A set is included exactly when its job
 * resolved true (the library's rule: a multi-set job all or nothing).  The handler runs before
 * the package's promises are settled, so a pool that merges here has the aggregate in place when
 * the caller's `await verifySignatureSets` continues.  A throwing (or rejecting) handler is
 * logged and never disturbs verdict delivery.
 */
function deliverAggregates(pkg, workResult, handler, logger) {
  try {
    const n = pkg.groupKeys.length;
    const tags = new Array(n);
    const jd = pkg.jobDesc;
    const groups = pkg.groups;
    let k = 0;
    for (let j = 0; j < pkg.nJobs; j++) {
      const nSets = jd[2 * j];
      if (workResult.status[j] === LSG_VALID) {
        for (let i = k; i < k + nSets; i++) {
          const g = groups[i];
          if (g === NO_GROUP) continue;
          if (tags[g] === undefined) tags[g] = [];
          tags[g].push(pkg.groupTags[i]);
        }
      }
      k += nSets;
    }
    const out = [];
    for (let g = 0; g < n; g++) {
      const count = workResult.aggCount[g];
      if (count === 0) continue;
      out.push({key: pkg.groupKeys[g], signature: workResult.agg.slice(96 * g, 96 * g + 96), count, tags: tags[g] || []});
    }
    if (out.length === 0) return;
    const r = handler(out);
    if (r && typeof r.then === "function") r.then(undefined, (e) => logger && logger.error("BlsGpuVerifier onAggregates error", {}, e));
  } catch (e) {
    if (logger) logger.error("BlsGpuVerifier onAggregates error", {}, e);
  }
}

/** GPU package policy defaults (see the class comment) */
const DEFAULT_MAX_SIGS_PER_PACKAGE = 32768;
const DEFAULT_EAGER_PACKAGES = 2;

class BlsGpuVerifier {
  /**
   * @param {{blsVerifyAllMultiThread?: boolean, device?: number, devices?: number[], seed?: number,
   *          maxSigsPerPackage?: number, eagerPackages?: number, minSigsWhenBusy?: number,
   *          maxPendingSigs?: number, bufferWaitMs?: number, reserveSets?: number,
   *          reservePubkeys?: number, reserveMsgBytes?: number, msgCacheEntries?: number,
   *          onAggregates?: (entries: {key: string, signature: Uint8Array, count: number, tags: any[]}[]) => void}} options
   *        onAggregates (SURVEY 8f(7)): with a handler, a set may carry `aggregateKey` (a string,
   *        e.g. the attestation data root) and `aggregateTag` (anything, e.g. the bit index): every
   *        package then also returns, per key, the compressed sum of the signatures of its sets
   *        that verified -- sets of different calls that share a key share a group -- and the
   *        handler gets one call per package, after the verdicts are known and before the
   *        package's promises are settled (deliverAggregates).  Without a handler the two fields
   *        are ignored and packages go out exactly as before.
   *        msgCacheEntries (default 0: off): rows of the per-device cache of hashed messages
   *        H(m) kept across packages -- a slot's AttestationData are hashed once, not once per
   *        package; 4096 holds three slots' worth with room for the singletons between them.
   * @param {{logger?: object, metrics?: object|null, addon?: object}} modules  addon is
   *        injectable (tests drive the queue logic with a mock of the addon's surface)
   *
   * Package policy (replaces the CPU pool's "<= 128 sigs per idle worker", index.ts:400-418,
   * whose 16 busy workers would hold the GPU to ~128-set packages and ~40k sets/s):
   *   - up to `eagerPackages` (2) packages go out as soon as jobs are queued, whatever their
   *     size: an idle GPU answers a lone job at once;
   *   - beyond that a package goes out only when the queue holds `minSigsWhenBusy` sigs
   *     (maxSigsPerPackage / 4), or when an in-flight package completes: while the GPU is
   *     busy the queue grows, so under load packages approach `maxSigsPerPackage` (32,768,
   *     one launch filling all 256 CUs) and light load keeps the latency of small packages;
   *   - at most one package per pipeline slot / package thread (addon.slots) is in flight.
   * Back-pressure (canAcceptWork, index.ts:143-149) is on SETS: queued + buffered + in flight
   * < `maxPendingSigs` (4 x maxSigsPerPackage: three to four packages on the GPU and one
   * filling; 5 x adds latency, not throughput: profiles/r06_node_ab.txt).  Per-job verdicts do
   * not depend on any of it: the GPU applies worker.ts's batch + retry rules to whatever
   * package it gets.
   * The reference's policy is {maxSigsPerPackage: 128, eagerPackages: slots}.
   */
  constructor(options = {}, modules = {}) {
    this.logger = modules.logger || null;
    this.metrics = modules.metrics || null;
    this.blsVerifyAllMultiThread = options.blsVerifyAllMultiThread === true;
    this.seed = options.seed || 0; // 0: randomizers from the OS CSPRNG (production)
    this.onAggregates = typeof options.onAggregates === "function" ? options.onAggregates : null;
    this.addon = modules.addon || loadAddon();
    // throws loudly without a gfx950 device
    this.ctx = this.addon.open(Array.isArray(options.devices) ? options.devices : options.device || 0);
    this.poolSize = this.addon.slots(this.ctx);
    this.maxSigsPerPackage = options.maxSigsPerPackage || DEFAULT_MAX_SIGS_PER_PACKAGE;
    this.eagerPackages = options.eagerPackages === undefined ? DEFAULT_EAGER_PACKAGES : options.eagerPackages;
    this.minSigsWhenBusy = options.minSigsWhenBusy || Math.max(1, Math.floor(this.maxSigsPerPackage / 4));
    this.maxPendingSigs = options.maxPendingSigs || 4 * this.maxSigsPerPackage;
    this.bufferWaitMs = options.bufferWaitMs === undefined ? MAX_BUFFER_WAIT_MS : options.bufferWaitMs;
    // the message cache (lsg_msg_cache_set), before the reservation, which sizes its buffers too
    this.msgCacheEntries = msgCacheOpen(this.addon, this.ctx, options.msgCacheEntries);
    if (options.reserveSets && this.addon.reserve) {
      // preallocate every pipeline slot for packages of up to reserveSets sets (lsg_reserve)
      const pks = options.reservePubkeys || options.reserveSets;
      // message bytes: 32 per set for signing roots; signingObject sets stage object + domain
      // (up to 160 bytes for an AttestationData, 296 for a ContributionAndProof, 16,761 for an
      // Electra AggregateAndProof): callers that send them say so (reserveMsgBytes)
      const msgBytes = options.reserveMsgBytes || 32 * options.reserveSets;
      this.addon.reserve(this.ctx, options.reserveSets, pks, msgBytes, this.poolSize);
    }
    this.jobs = new Fifo(); // queued pages (index.ts `jobs`)
    this.priorityPages = []; // pages of priority jobs: a stack, drained first
    this.tail = null; // the last queued page while it accepts jobs
    this.buffer = null; // buffered batchable jobs (index.ts `bufferedJobs`), a page not yet queued
    this.queuedJobs = 0;
    this.queuedSigs = 0;
    this.closed = false;
    this.workersBusy = 0; // packages in flight (the reference's busy workers)
    this.sigsInFlight = 0;
    this.inflight = new Set();
    this.spare = []; // packed buffers of completed packages, reused
    this.stats = {packages: 0, packageSigs: 0}; // packages submitted and their sets (bench, tests)
    this.scheduled = false;
    this.kick = false; // a package completed: the next dispatch goes out whatever its size
    this._runJob = this._runJob.bind(this);
    this._runBufferedJobs = this._runBufferedJobs.bind(this);
    this._onBufferTimer = this._onBufferTimer.bind(this);
    this.bufferTimer = null;
    const m = this.metrics && this.metrics.blsThreadPool;
    if (m && m.queueLength && m.workersBusy && typeof m.queueLength.addCollect === "function") {
      // index.ts:135-140: sampled at scrape time
      m.queueLength.addCollect(() => {
        m.queueLength.set(this.queuedJobs);
        m.workersBusy.set(this.workersBusy);
      });
    }
  }

  /** Mirror index2pubkey[firstIndex ..] into the device pubkey table (SURVEY 8f(1); call next
   * to pubkeyCache.ts syncPubkeys / epochContext.ts addPubkey).  Sets may then carry
   * `pubkeyIndices` instead of PublicKeys.  Returns per-key BLST codes (0 = loaded). */
  loadPubkeys(firstIndex, pubkeys) {
    return this.addon.pubkeyTableSet(this.ctx, firstIndex, pubkeys.map(pubkeyBytes));
  }

  /** The message cache's counters summed over the devices (lsg_msg_cache_get_stats): lookups,
   * hits, pending, inserts, evictions, bypassed, full, entries, capacity -- all 0 with
   * msgCacheEntries 0. */
  getMsgCacheStats() {
    if (this.closed) throw new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    return msgCacheStatsSync(this.addon, this.ctx);
  }

  /** Register committees on the device (SURVEY 8f(5); call where the node fills its shuffling
   * and sync-committee caches): committee firstId + c <- committees[c], validator indices in
   * committee order (rows loaded with loadPubkeys).  An aggregate set may then carry
   * {committee, bits, bitLen} instead of pubkeys or pubkeyIndices, or -- an Electra aggregate
   * spanning committees -- {committees, bits, bitLen}: up to 64 ids and one bitfield over the
   * concatenation of those committees.  Returns per-committee codes
   * (0 = registered; 102: a member names an unloaded index; 101: an empty committee). */
  loadCommittees(firstId, committees) {
    return loadCommitteesSync(this.addon, this.ctx, firstId, committees);
  }

  /** Unset committees firstId .. firstId + n - 1 (an epoch's committees that are no longer used). */
  clearCommittees(firstId, n) {
    if (typeof this.addon.committeesClear !== "function") throw Error("the addon does not support clearCommittees");
    this.addon.committeesClear(this.ctx, firstId, n);
  }

  /** Op-pool aggregation (SURVEY 8f(4)): bls.Signature.aggregate(sigs.map(signatureFromBytesNoCheck))
   * .toBytes() of opPools/attestationPool.ts:195, syncCommitteeMessagePool.ts:139,
   * aggregatedAttestationPool.ts:322 and syncContributionAndProofPool.ts:185, for many groups in
   * one device pass.  Returns [{signature: Uint8Array(96) | null, err}] per group; err is the
   * BLST code of the group's first undecodable signature (101 = EMPTY_AGGREGATE_ARRAY). */
  aggregateSignatures(groups) {
    return this.addon.aggregateSignatures(this.ctx, groups);
  }

  /** processDeposit.ts:47-66 for a list of deposits (verifyDepositsSync above): domain is
   * computeDomain(DOMAIN_DEPOSIT, GENESIS_FORK_VERSION, ZERO_HASH); resolves to boolean[]. */
  async verifyDeposits(depositDatas, domain) {
    if (this.closed) throw new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    return verifyDepositsSync(this.addon, this.ctx, depositDatas, domain);
  }

  /** Sets not yet answered: queued, buffered and on the GPU. */
  pendingSigs() {
    return this.queuedSigs + (this.buffer ? this.buffer.nSigs : 0) + this.sigsInFlight;
  }

  canAcceptWork() {
    return this.pendingSigs() < this.maxPendingSigs;
  }

  verifySignatureSets(sets, opts = {}) {
    try {
      if (this.metrics && this.metrics.bls) this.metrics.bls.aggregatedPubkeys.inc(getAggregatedPubkeysCount(sets));

      if (opts.verifyOnMainThread && !this.blsVerifyAllMultiThread) {
        // verifySignatureSetsMaybeBatch without the queue: no retry, errors reject
        const m = this.metrics && this.metrics.blsThreadPool;
        const timer = m ? m.mainThreadDurationInThreadPool.startTimer() : null;
        const p = verifyDirect(this.addon, this.ctx, sets, this.seed, opts.validatePubkeys === true, this.onAggregates, this.logger);
        if (timer) p.then(timer, timer);
        return p;
      }

      for (let i = 0; i < sets.length; i++) checkSet(sets[i]);
      // one chunk (the common case: a gossip call carries one set): the AND over one job's
      // boolean verdict is that verdict, so the job's own promise is the answer
      if (sets.length <= MAX_SIGNATURE_SETS_PER_JOB) return this._queueBlsWork(opts, sets);
      return Promise.all(
        chunkifyMaximizeChunkSize(sets, MAX_SIGNATURE_SETS_PER_JOB).map((setsWorker) => this._queueBlsWork(opts, setsWorker))
      ).then((results) => {
        // .every on an empty array returns true
        if (results.length === 0) {
          throw Error("Empty results array");
        }
        return results.every((isValid) => isValid === true);
      });
    } catch (e) {
      return Promise.reject(e);
    }
  }

  /**
   * Per-set verdicts for sets that share one message (north-star extension).  The sets go
   * out as one package of single-set batchable jobs: the GPU verifies them as one RLC batch
   * and, if that fails, re-verifies each set on its own (worker.ts:74-96).  A set whose
   * signature does not decode is reported false.
   */
  verifySignatureSetsSameMessage(sets, message, opts = {}) {
    const o = {batchable: true, priority: opts.priority};
    return Promise.all(
      sets.map((s) =>
        this._queueBlsWork(o, [
          s.committees !== undefined
            ? {
                // an aggregate spanning committees goes through as it is
                committees: s.committees,
                bits: s.bits,
                bitLen: s.bitLen,
                signingRoot: message,
                signature: s.signature,
                aggregateKey: s.aggregateKey,
                aggregateTag: s.aggregateTag,
              }
            : {
                type: SignatureSetType.single,
                pubkey: s.publicKey,
                signingRoot: message,
                signature: s.signature,
                aggregateKey: s.aggregateKey,
                aggregateTag: s.aggregateTag,
              },
        ]).catch(() => false)
      )
    );
  }

  async close() {
    const aborted = new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    if (this.bufferTimer) {
      clearTimeout(this.bufferTimer);
      this.bufferTimer = null;
    }
    if (this.buffer) {
      this.buffer.failRest(aborted);
      this.buffer = null;
    }
    for (const pg of this.priorityPages) pg.failRest(aborted);
    for (const pg of this.jobs.drain()) pg.failRest(aborted);
    this.priorityPages = [];
    this.tail = null;
    this.queuedJobs = 0;
    this.queuedSigs = 0;
    this.closed = true;
    // let packages already on the GPU finish, then release the device context
    await Promise.all(Array.from(this.inflight));
    if (this.ctx) {
      this.addon.close(this.ctx);
      this.ctx = null;
    }
  }

  _queueBlsWork(opts, sets) {
    if (this.closed) {
      return Promise.reject(new QueueError({code: QueueErrorCode.QUEUE_ABORTED}));
    }
    const added = this.metrics !== null;
    const validate = opts.validatePubkeys === true;
    if (opts.priority === true) {
      // north-star extension: the job goes to the head of the queue, not through the buffer
      const page = new JobPage(opts.batchable === true, true, added ? [] : null, validate);
      const p = page.push(sets);
      page.open = false;
      this.priorityPages.push(page);
      this.queuedJobs++;
      this.queuedSigs += sets.length;
      this._schedule();
      return p;
    }
    if (opts.batchable === true) {
      const tail = this.tail;
      if (tail !== null && tail.batchable && tail.open && tail.validate === validate) {
        // the buffer was flushed and is still waiting in the queue: join it there
        const p = tail.push(sets);
        this.queuedJobs++;
        this.queuedSigs += sets.length;
        this._schedule();
        return p;
      }
      let buf = this.buffer;
      if (buf !== null && buf.validate !== validate) {
        // the buffer holds the other kind: it goes to the queue as it is, a new one opens
        this._runBufferedJobs();
        buf = null;
      }
      if (buf === null) {
        buf = this.buffer = new JobPage(true, false, added ? [] : null, validate);
        buf.firstPush = Date.now();
        this._armBufferTimer();
      }
      const p = buf.push(sets);
      if (buf.nSigs > MAX_BUFFERED_SIGS || !buf.open) this._runBufferedJobs();
      return p;
    }
    let page = this.tail;
    if (page === null || page.batchable || !page.open || page.validate !== validate) {
      page = new JobPage(false, false, added ? [] : null, validate);
      this.jobs.push(page);
      this.tail = page;
    }
    const p = page.push(sets);
    this.queuedJobs++;
    this.queuedSigs += sets.length;
    this._schedule();
    return p;
  }

  /** One timer for the buffer's 100 ms limit (index.ts:291-293 arms one per buffer; a buffer
   * that fills first would cost a setTimeout + clearTimeout pair per ~33 sigs): on firing it
   * flushes the buffer if it is old enough, else re-arms for the rest of its wait. */
  _armBufferTimer() {
    if (!this.bufferTimer) this.bufferTimer = setTimeout(this._onBufferTimer, this.bufferWaitMs);
  }

  _onBufferTimer() {
    this.bufferTimer = null;
    const buf = this.buffer;
    if (!buf) return;
    const age = Date.now() - buf.firstPush;
    if (age >= this.bufferWaitMs) this._runBufferedJobs();
    else this.bufferTimer = setTimeout(this._onBufferTimer, this.bufferWaitMs - age);
  }

  _schedule() {
    // setImmediate, not the reference's setTimeout(0) (a >= 1 ms timer in node)
    if (!this.scheduled) {
      this.scheduled = true;
      setImmediate(this._runJob);
    }
  }

  _runJob() {
    this.scheduled = false;
    if (this.closed) return;
    while (this.workersBusy < this.poolSize && this.queuedJobs > 0) {
      // while the GPU is busy let the queue grow into a large package, unless a package has
      // just completed (class comment)
      if (this.workersBusy >= this.eagerPackages && this.queuedSigs < this.minSigsWhenBusy && !this.kick) break;
      this.kick = false;
      const work = this._prepareWork();
      if (work.ranges.length === 0) break;
      this._runPackage(work);
    }
  }

  _runPackage(work) {
    const m = this.metrics && this.metrics.blsThreadPool;
    const ranges = work.ranges;
    const startedSigSets = work.nSigs;
    if (m) {
      const now = Date.now();
      for (let r = 0; r < ranges.length; r += 3) {
        const added = ranges[r].added;
        for (let j = ranges[r + 1]; j < ranges[r + 2]; j++) m.jobWaitTime.observe((now - added[j]) / 1000);
      }
      m.totalJobsGroupsStarted.inc(1);
      m.totalJobsStarted.inc(work.nJobs);
      m.totalSigSetsStarted.inc(startedSigSets);
    }
    this.workersBusy++;
    this.sigsInFlight += startedSigSets;
    this.stats.packages++;
    this.stats.packageSigs += startedSigSets;
    const run = (async () => {
      let pkg = null;
      try {
        // buffers sized for a full package, so that every one can be reused
        pkg = packJobs(ranges, startedSigSets, this.spare.pop(), this.maxSigsPerPackage, this.onAggregates !== null);
        if (pkg.nJobs === 0) return;
        const jobStartNs = process.hrtime.bigint();
        const workResult =
          pkg.groups === null
            ? await this.addon.verifyPacked(this.ctx, pkg.arena, pkg.setDesc, pkg.jobDesc, this.seed)
            : await this.addon.verifyPacked(this.ctx, pkg.arena, pkg.setDesc, pkg.jobDesc, this.seed, false, pkg.groups, pkg.groupKeys.length);
        const jobEndNs = process.hrtime.bigint();
        if (m) {
          // index.ts:362-381, with the GPU package in the worker's place
          let errorCount = 0;
          const jd = pkg.jobDesc;
          for (let i = 0; i < pkg.nJobs; i++) if (workResult.status[i] === LSG_ERROR) errorCount += jd[2 * i];
          const workerJobTimeSec = (workResult.endNs - workResult.startNs) / 1e9;
          const latencyToWorkerSec = (workResult.startNs - Number(jobStartNs)) / 1e9;
          const latencyFromWorkerSec = (Number(jobEndNs) - workResult.endNs) / 1e9;
          m.timePerSigSet.observe(workerJobTimeSec / startedSigSets);
          m.jobsWorkerTime.inc({workerId: workResult.workerId || 0}, workerJobTimeSec);
          m.latencyToWorker.observe(latencyToWorkerSec);
          m.latencyFromWorker.observe(latencyFromWorkerSec);
          m.successJobsSignatureSetsCount.inc(pkg.nSigs - errorCount);
          m.errorJobsSignatureSetsCount.inc(errorCount);
          m.batchRetries.inc(workResult.batchRetries);
          m.batchSigsSuccess.inc(workResult.batchSigsSuccess);
        }
        if (pkg.groups !== null) deliverAggregates(pkg, workResult, this.onAggregates, this.logger);
        settleJobs(ranges, workResult.status, workResult.errCode);
        if (this.spare.length < this.poolSize) this.spare.push(pkg);
      } catch (e) {
        if (!this.closed && this.logger) this.logger.error("BlsGpuVerifier error", {}, e);
        failJobs(ranges, e);
      }
    })();
    this.inflight.add(run);
    run.then(() => {
      this.inflight.delete(run);
      this.workersBusy--;
      this.sigsInFlight -= startedSigSets;
      this.kick = true;
      this._schedule();
    });
  }

  /** Jobs for one package: priority pages first, then FIFO, up to maxSigsPerPackage sigs, a
   * job at a time as index.ts:400-418 takes them (a page may be split between packages). */
  _prepareWork() {
    const ranges = [];
    let totalSigs = 0;
    let totalJobs = 0;
    const max = this.maxSigsPerPackage;
    while (totalSigs < max) {
      const prio = this.priorityPages.length > 0;
      const page = prio ? this.priorityPages[this.priorityPages.length - 1] : this.jobs.peek();
      if (page === undefined) break;
      page.open = false;
      if (page === this.tail) this.tail = null;
      const start = page.taken;
      let end = start;
      if (!page.multi) {
        // single-set jobs (the gossip shape): one sig per job
        end = Math.min(page.n, start + (max - totalSigs));
        totalSigs += end - start;
      } else {
        const sets = page.sets;
        while (end < page.n && totalSigs < max) totalSigs += sets[end++].length;
      }
      page.taken = end;
      totalJobs += end - start;
      ranges.push(page, start, end);
      if (end === page.n) {
        if (prio) this.priorityPages.pop();
        else this.jobs.shift();
      }
    }
    this.queuedSigs -= totalSigs;
    this.queuedJobs -= totalJobs;
    return {ranges, nSigs: totalSigs, nJobs: totalJobs};
  }

  _runBufferedJobs() {
    const buf = this.buffer;
    if (buf) {
      // the buffer goes to the tail of the queue as a whole (index.ts:425-431)
      this.buffer = null;
      this.jobs.push(buf);
      this.tail = buf;
      this.queuedJobs += buf.n;
      this.queuedSigs += buf.nSigs;
      this._schedule();
    }
  }
}

/**
 * BlsSingleThreadVerifier (chain/bls/singleThread.ts:14-35) on the GPU: each call is one
 * verifySignatureSetsMaybeBatch (verifyDirect: one priority job, no queue) with no retry; opts
 * are ignored but for opts.validatePubkeys (the job carries JOB_VALIDATE_KEYS: an object's own
 * key is validated whichever verifier createBlsVerifier chose), errors reject.  The reference blocks the event loop for the call; here the
 * promise settles when the GPU answers.  The duration is observed after the call as the
 * reference does (it observes the total and the per-set time; its startNs - endNs has the
 * sign inverted, here the duration is positive).
 */
class BlsGpuSingleThreadVerifier {
  /**
   * @param {{device?: number, devices?: number[], seed?: number, msgCacheEntries?: number}} options
   * @param {{metrics?: object|null, addon?: object}} modules
   */
  constructor(options = {}, modules = {}) {
    this.metrics = modules.metrics || null;
    this.seed = options.seed || 0;
    this.addon = modules.addon || loadAddon();
    this.ctx = this.addon.open(Array.isArray(options.devices) ? options.devices : options.device || 0);
    this.msgCacheEntries = msgCacheOpen(this.addon, this.ctx, options.msgCacheEntries);
  }

  /** as BlsGpuVerifier.getMsgCacheStats */
  getMsgCacheStats() {
    if (!this.ctx) throw new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    return msgCacheStatsSync(this.addon, this.ctx);
  }

  async verifySignatureSets(sets, opts = {}) {
    if (this.metrics && this.metrics.bls) this.metrics.bls.aggregatedPubkeys.inc(getAggregatedPubkeysCount(sets));
    for (let i = 0; i < sets.length; i++) if (sets[i].signingObject !== undefined) checkMsgObject(sets[i]);
    // Count time after aggregating (serialisation happens inside verifyDirect)
    const startNs = process.hrtime.bigint();
    const valid = await verifyDirect(this.addon, this.ctx, sets, this.seed, opts.validatePubkeys === true);
    // Don't use a try/catch, only count run without exceptions
    const endNs = process.hrtime.bigint();
    const totalSec = Number(endNs - startNs) / 1e9;
    const m = this.metrics && this.metrics.blsThreadPool;
    if (m) {
      m.mainThreadDurationInThreadPool.observe(totalSec);
      m.mainThreadDurationInThreadPool.observe(totalSec / sets.length);
    }
    return valid;
  }

  /** as BlsGpuVerifier.loadCommittees */
  loadCommittees(firstId, committees) {
    if (!this.ctx) throw new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    return loadCommitteesSync(this.addon, this.ctx, firstId, committees);
  }

  /** processDeposit.ts:47-66 for a list of deposits, as BlsGpuVerifier.verifyDeposits */
  async verifyDeposits(depositDatas, domain) {
    if (!this.ctx) throw new QueueError({code: QueueErrorCode.QUEUE_ABORTED});
    return verifyDepositsSync(this.addon, this.ctx, depositDatas, domain);
  }

  async close() {
    if (this.ctx) {
      this.addon.close(this.ctx);
      this.ctx = null;
    }
  }

  canAcceptWork() {
    // Since sigs are verified blocking the main thread, there's no mechanism to throttle
    return true;
  }
}

/** chain.ts:195-198: opts.blsVerifyAllMainThread selects the single-thread verifier. */
function createBlsVerifier(opts = {}, modules = {}) {
  return opts.blsVerifyAllMainThread ? new BlsGpuSingleThreadVerifier(opts, modules) : new BlsGpuVerifier(opts, modules);
}

module.exports = {
  BlsGpuVerifier,
  BlsGpuSingleThreadVerifier,
  createBlsVerifier,
  QueueError,
  QueueErrorCode,
  SignatureSetType,
  chunkifyMaximizeChunkSize,
  errorMessage,
  packJobs,
  getAggregatedPubkeysCount,
  DEFAULT_MAX_SIGS_PER_PACKAGE,
  MAX_SIGNATURE_SETS_PER_JOB,
  MAX_BUFFERED_SIGS,
  MAX_BUFFER_WAIT_MS,
  MAX_JOBS_CAN_ACCEPT_WORK,
};
