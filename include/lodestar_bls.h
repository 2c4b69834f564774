/*
 * lodestar_bls.h -- C ABI of the MI355X (gfx950) BLS12-381 signature-set verifier.
 *
 * Drop-in boundary for Lodestar's IBlsVerifier hot path
 * (/root/reference/packages/beacon-node/src/chain/bls/interface.ts:20-51).  It replaces
 * the worker threads of BlsMultiThreadWorkerPool together with the crypto library they
 * call (@chainsafe/bls@7.1.1 -> @chainsafe/blst@0.2.8 -> supranational blst):
 *
 *   lsg_verify_jobs        <- multithread/worker.ts:30-106 verifyManySignatureSets
 *                             (+ maybeBatch.ts:16-39 verifySignatureSetsMaybeBatch,
 *                                worker.ts:108-114 deserializeSet)
 *   lsg_verify_sets        <- maybeBatch.ts:16-39 for one call (BlsSingleThreadVerifier,
 *                             singleThread.ts:14-35; verifyOnMainThread, index.ts:155-168)
 *   lsg_aggregate_pubkeys  <- utils.ts:11 PublicKey.aggregate (+ toBytes, index.ts:177)
 *   lsg_hash_to_g2         <- blst Hash_to_G2 inside Pairing.mul_n_aggregate
 *   lsg_sig_decode         <- maybeBatch.ts:23,36 Signature.fromBytes(bytes, affine, true)
 *   lsg_aggregate_signatures <- opPools Signature.aggregate
 *   lsg_*signing_roots     <- util/signingRoot.ts:7-13 computeSigningRoot
 *   lsg_verify_deposits    <- block/processDeposit.ts:47-66 (KeyValidate + verify per deposit)
 *   lsg_submit_jobs /      <- the asynchronous lsg_submit / lsg_wait pair of SURVEY.md 8b:
 *   lsg_wait_jobs             one BlsWorkReq[] package in flight per pipeline slot
 *   lsg_init_devices       <- the node-wide pool (chain.ts:195-198, multithread/poolSize.ts:7):
 *                             one context over every GPU of the node
 *   lsg_jobs_partial /     <- the per-GPU half of a package for one-process-per-GPU hosts
 *   lsg_wait_jobs_node        (SURVEY.md 8e): Miller-loop product of the package group,
 *   lsg_batch_partial /       all-gathered by the caller, one final exponentiation
 *   lsg_final_*               (lsg_final_*), then the verdicts resolved with it
 *
 * Plain pointers and sizes only; every call returns an int status (LSG_OK = 0) and never
 * throws.  Verdicts and error codes follow blst's numbering (BLST_* below).  All compute
 * runs in HIP kernels on the context's device; there is no CPU fallback -- lsg_init fails
 * with LSG_ERR_NO_DEVICE when no gfx950 device is present.
 */
#ifndef LODESTAR_BLS_H
#define LODESTAR_BLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- call status */
#define LSG_OK 0
#define LSG_ERR_INVALID_ARG 1
#define LSG_ERR_NO_DEVICE 2
#define LSG_ERR_DEVICE 3
#define LSG_ERR_NOMEM 4
#define LSG_ERR_CLOSED 5
#define LSG_ERR_BUSY 6 /* every pipeline slot holds an outstanding ticket (canAcceptWork false) */
#define LSG_ERR_ENTROPY 7 /* the OS CSPRNG (getrandom) failed: no RLC randomizers, nothing verified */

/* ---- blst error codes (blst.h BLST_ERROR) + @chainsafe/blst's size error */
#define LSG_BLST_SUCCESS 0
#define LSG_BLST_BAD_ENCODING 1
#define LSG_BLST_POINT_NOT_ON_CURVE 2
#define LSG_BLST_POINT_NOT_IN_GROUP 3
#define LSG_BLST_AGGR_TYPE_MISMATCH 4
#define LSG_BLST_VERIFY_FAIL 5
#define LSG_BLST_PK_IS_INFINITY 6
#define LSG_BLST_BAD_SCALAR 7
#define LSG_BLST_INVALID_SIZE 10
/* non-blst job errors */
#define LSG_ERR_EMPTY_SET 100        /* maybeBatch.ts:29-31 "Empty signature set" */
#define LSG_ERR_EMPTY_AGGREGATE 101  /* PublicKey.aggregate([]) "EMPTY_AGGREGATE_ARRAY" */
#define LSG_ERR_BAD_INDEX 102        /* a pubkey index outside the loaded table (index2pubkey[i] undefined) */
#define LSG_ERR_BAD_COMMITTEE 103    /* unknown / unset committee id, or n_pks != its length */

/* lsg_set.pk_len value for keys given by validator index into the context's pubkey table
 * (lsg_pubkey_table_set): pks then points at n_pks uint32 indices (host byte order). */
#define LSG_PK_INDEX 4u
/* lsg_set.pk_len value for keys named by committee id + participation bits (lsg_committees_set):
 * n_pks is the bit count and must equal the committee's length; pks points at
 * 4 + ceil(n_pks / 8) bytes: the uint32 committee id (host byte order), then the bitfield in SSZ
 * order without a delimiter bit -- member k is bit k & 7 of byte k >> 3; bits at positions
 * >= n_pks are ignored.  The set behaves exactly as the same set with LSG_PK_INDEX and the
 * participating members' table indices in committee order: no bit set is
 * LSG_ERR_EMPTY_AGGREGATE as n_pks == 0 is; an unknown id, an unset committee or a length
 * mismatch is LSG_ERR_BAD_COMMITTEE, routed exactly like LSG_ERR_BAD_INDEX (a deserializeSet
 * failure: the package is rejected, lsg_stats.key_error / key_error_job say where).  Honoured
 * wherever sets are staged -- lsg_submit_jobs / lsg_wait_jobs / lsg_verify_jobs,
 * lsg_verify_sets, lsg_aggregate_pubkeys_multi, lsg_batch_partial, coalesced packages, every
 * device of a multi-device context, the node protocol -- and a package may mix byte, index and
 * bits sets.  lsg_aggregate_pubkeys (one key list) does not take it: 8 stays an unknown key
 * length there.  LSG_JOB_VALIDATE_KEYS leaves such sets alone, as it leaves index sets alone. */
#define LSG_PK_BITS 8u
/* lsg_set.pk_len value for keys named by a LIST of committees + one participation bitfield over
 * their concatenation (an EIP-7549 aggregate: committee_bits + aggregation_bits).  n_pks is the
 * total bit count; pks points at 4 + 4 k + ceil(n_pks / 8) bytes, no alignment assumed: a uint32
 * k, the number of committees (host byte order), then k uint32 committee ids as registered with
 * lsg_committees_set, then the bitfield in SSZ order without a delimiter bit.  Bit off_c + i is
 * member i of the c-th listed committee, off_c the sum of the lengths of the committees listed
 * before it; bits at positions >= n_pks are ignored, whatever they hold.  The set behaves exactly
 * as the same set with LSG_PK_INDEX and the participating members' table indices, in list order
 * and then committee order -- aggregates, verdicts, error codes and their precedence, batch
 * counters, lsg_stats, exported partials and grouped aggregates.  Ids may repeat and need not
 * ascend; a listed committee may have no participant.
 *   LSG_ERR_BAD_COMMITTEE (routed exactly like LSG_ERR_BAD_INDEX, as for LSG_PK_BITS): a listed id
 *     is unknown or unset, n_pks differs from the sum of the listed committees' lengths, or
 *     k == 0 with n_pks > 0;
 *   LSG_ERR_EMPTY_AGGREGATE: no bit set among the first n_pks (k == 0, n_pks == 0 included);
 *   LSG_ERR_INVALID_ARG from the entry point, with nothing staged and the context usable:
 *     k > LSG_MAX_SET_COMMITTEES or pks == NULL (caller bugs, as a bad LSG_MSG_OBJECT length is).
 * Honoured wherever LSG_PK_BITS is, and a package may mix byte, index, bits and multi sets
 * (aggregated by k_pk_agg_bits_multi, launched only by packages that hold such a set).
 * lsg_aggregate_pubkeys (one key list) does not take it: 12 stays an unknown key length there.
 * LSG_JOB_VALIDATE_KEYS leaves such sets alone. */
#define LSG_PK_BITS_MULTI 12u
#define LSG_MAX_SET_COMMITTEES 64u

/* or'ed into lsg_set.msg_len: msg points at an SSZ-serialized object followed by its 32-byte
 * domain; the message signed is computeSigningRoot(object, domain)
 * (state-transition/src/util/signingRoot.ts:7-13), computed on the device as the package's first
 * stage (k_msg_roots).  A marked msg_len is read in three fields: bit 31 the
 * marker, bits 24..30 a kind tag (LSG_MSG_KIND_MASK), bits 0..23 the payload length (object +
 * domain).  An unmarked length is a byte count in all its bits.  With tag 0 the payload length
 * selects the kind:
 *    40  uint64 (Slot, Epoch: randao reveal, selection proof)
 *    48  two uint64 fields (phase0.VoluntaryExit; altair.SyncAggregatorSelectionData)
 *    64  Root (any object whose hashTreeRoot the caller has: block proposer, sync committee)
 *   108  capella.BLSToExecutionChange (validatorIndex u64, fromBlsPubkey 48, toExecutionAddress 20)
 *   120  phase0.DepositMessage (pubkey 48, withdrawalCredentials 32, amount u64)
 *   144  phase0.BeaconBlockHeader (slot, proposerIndex, parentRoot, stateRoot, bodyRoot)
 *   160  phase0.AttestationData (slot, index, beaconBlockRoot, source, target)
 *   296  altair.ContributionAndProof (aggregatorIndex u64, contribution 160, selectionProof 96)
 * A non-zero tag names a variable-size kind, whose root k_msg_roots_var computes with one 64-lane
 * workgroup per message:
 *   LSG_MSG_KIND_AGG_PROOF          phase0.AggregateAndProof (Attestation with Bitlist[2048]):
 *                                   object 337..593 bytes
 *   LSG_MSG_KIND_AGG_PROOF_ELECTRA  EIP-7549's AggregateAndProof (Attestation {aggregation_bits:
 *                                   Bitlist[131072], data, signature, committee_bits:
 *                                   Bitvector[64]}): object 345..16,729 bytes
 * serialized as aggregatorIndex [0,8), offset 108 [8,12), selectionProof [12,108), inner offset
 * [108,112) (228, Electra 236), AttestationData [112,240), signature [240,336), Electra's
 * committee_bits [336,344), then the bitlist with its delimiter bit (1..257 bytes, Electra
 * 1..16,385).  Wrong offsets, a zero last byte, more bits than the limit, a length outside the
 * range or another tag are caller bugs as a bad tag-0 length is.  These payloads exceed the
 * message cache's 192 bytes and are counted as `bypassed`.
 * Such a set behaves exactly as the same set with msg = the 32-byte signing root and msg_len = 32:
 * verdicts, error codes and their precedence, the batch counters and the exported partial.
 * Honoured wherever sets are staged with a message -- lsg_submit_jobs / lsg_wait_jobs /
 * lsg_verify_jobs, lsg_verify_sets, lsg_batch_partial, coalesced packages, every device of a
 * multi-device context, the node protocol; a package, and a job, may mix object sets with plain
 * messages of any length, and the form combines with byte, index and bits keys and with
 * LSG_JOB_VALIDATE_KEYS.  A marked set with another payload length or with msg == NULL is a
 * caller bug, not data: the entry point returns LSG_ERR_INVALID_ARG before anything is staged
 * and the context stays usable.  lsg_hash_to_g2 and lsg_sign reject a marked length with
 * LSG_ERR_INVALID_ARG; lsg_aggregate_pubkeys_multi ignores messages as before.  Messages are
 * deduplicated on the staged bytes (object, domain and marker): sets naming the same object and
 * domain share one root, one hash_to_G2 and one Miller pair.  The payload bytes count toward
 * lsg_reserve's max_msg_bytes.  A package with no marked set stages, allocates and launches
 * exactly what it did without the form. */
#define LSG_MSG_OBJECT 0x80000000u
#define LSG_MSG_KIND_SHIFT 24
#define LSG_MSG_KIND_MASK 0x7f000000u
#define LSG_MSG_KIND_AGG_PROOF 1u
#define LSG_MSG_KIND_AGG_PROOF_ELECTRA 2u

/* ---- job verdicts (WorkResult<boolean>, multithread/types.ts:21-24) */
#define LSG_INVALID 0 /* {code: success, result: false} */
#define LSG_VALID 1   /* {code: success, result: true}  */
#define LSG_ERROR 2   /* {code: error, error}           */

/* ---- job flags (VerifySignatureOpts, interface.ts:3-18; priority/same-message are extensions) */
#define LSG_JOB_BATCHABLE 1u
/* A package with a priority job (verifyOnMainThread, BlsGpuSingleThreadVerifier) is never held
 * by coalescing and runs on its slot's high-priority streams: its kernels are dispatched ahead
 * of the packages in flight.  Verdicts are unaffected. */
#define LSG_JOB_PRIORITY 2u
/* The job's sets carry their own, untrusted public keys (deposits, processDeposit.ts:57;
 * BLS-to-execution changes, signatureSets/blsToExecutionChange.ts:32): every byte key (48 or 96
 * bytes) of every set of the job is run through KeyValidate on the device, inside the package's
 * pipeline -- decode, not infinity (BLST_PK_IS_INFINITY), in the r-torsion subgroup
 * (BLST_POINT_NOT_IN_GROUP); the codes of lsg_pubkey_validate, BLST_INVALID_SIZE for another
 * length.  A key that fails is its SET's error, routed like a signature that does not decode:
 * the job resolves to LSG_ERROR with the code (inside a set the key's code beats the
 * signature's, in an aggregate set the first bad key in order gives it; inside a job the first
 * set in order that has an error does), the set stays out of every RLC group, the other jobs
 * keep their verdicts, lsg_stats.key_error stays 0 and the batch counters count the set as a
 * per-set error.  Keys named by table index (LSG_PK_INDEX) are left alone.  Honoured wherever
 * jobs go: lsg_submit_jobs / lsg_wait_jobs / lsg_verify_jobs, coalesced packages, every device
 * of a multi-device context, the node protocol.  A package with no such job launches, stages
 * and allocates exactly what it did without the flag. */
#define LSG_JOB_VALIDATE_KEYS 4u

typedef struct lsg_ctx lsg_ctx;
typedef uint64_t lsg_ticket; /* handle of an in-flight submission */

/* One signature set (ISignatureSet, state-transition/src/util/signatureSets.ts:10-22).
 * Pubkeys are the set's n_pks keys back to back, each pk_len bytes (48 compressed or
 * 96 uncompressed, ZCash encoding).  n_pks == 1 is a "single" set, > 1 an "aggregate"
 * set whose keys are summed on the GPU.  sig_len other than 96/192 yields
 * BLST_INVALID_SIZE for the set, exactly as Signature.fromBytes does. */
typedef struct {
  const uint8_t* pks;
  uint32_t pk_len;
  uint32_t n_pks;
  const uint8_t* msg;
  uint32_t msg_len;
  const uint8_t* sig;
  uint32_t sig_len;
} lsg_set;

/* One job = one BlsWorkReq (multithread/types.ts:14-17): the sets of one
 * verifySignatureSets chunk (<= 128 sets) plus its options. */
typedef struct {
  const lsg_set* sets;
  uint32_t n_sets;
  uint32_t flags;
} lsg_job;

typedef struct {
  int32_t status;   /* LSG_VALID / LSG_INVALID / LSG_ERROR */
  int32_t err_code; /* BLST_* or LSG_ERR_EMPTY_* when status == LSG_ERROR */
} lsg_job_result;

/* BlsWorkResult counters (multithread/types.ts:26-38) */
typedef struct {
  uint32_t batch_retries;
  uint32_t batch_sigs_success;
  uint64_t start_ns;      /* CLOCK_MONOTONIC ns (process.hrtime's clock): submit entered */
  uint64_t end_ns;        /* CLOCK_MONOTONIC ns: verdicts resolved */
  uint32_t n_final_exps;  /* final exponentiations run (package, chunk and job groups; node check) */
  uint32_t submit_us;     /* host time inside lsg_submit_jobs (staging, randomizers, plans, launches) */
  int32_t key_error;      /* deserializeSet failure that rejected the whole package (BLST_*), 0: none */
  uint32_t key_error_job; /* caller index of the job holding that first bad key */
} lsg_stats;

/* A context over one or more devices.  Per device it owns 16 pipeline slots (each: a main
 * and a side HIP stream plus its own device buffers; lsg_pipeline_slots), and device 0 owns
 * 64 final-exponentiation entries on 8 streams (lsg_final_*).  Calls are serialised by an
 * internal mutex; waits block without holding it.
 *   lsg_init(d)              one device (d < 0: device 0)
 *   lsg_init_devices(ids, n) the node's GPUs (chain.ts:195-198 builds ONE verifier per node;
 *                            its pool spans every core, multithread/poolSize.ts:7).  A package
 *                            is split into whole jobs by cumulative set count; each device
 *                            reduces its share to one Fp12 partial, the partials are
 *                            all-gathered over RCCL (communicators owned by the context) and
 *                            one final exponentiation on device 0 checks the node; on failure
 *                            every device localises with its own check.
 *                            Duplicate ids (tests) exchange by device copies instead. */
int lsg_init(int device_ordinal, lsg_ctx** out);
int lsg_init_devices(const int* device_ids, int n_devices, lsg_ctx** out);
int lsg_destroy(lsg_ctx* ctx);
int lsg_device_count(lsg_ctx* ctx, int32_t* n);
const char* lsg_last_error(lsg_ctx* ctx);
int lsg_device_name(lsg_ctx* ctx, char* buf, size_t len);
/* Preallocate every device and pinned buffer of the first n_slots pipeline slots (0 = all) of
 * every device for packages of up to max_sets sets, max_pks keys and max_msg_bytes message
 * bytes, so that submissions within those bounds allocate nothing.  A context over n devices
 * reserves each device for its share: 1/n of each bound plus one 4,096-set job's worth.
 * lsg_submit_jobs stages a package with the context lock released (several host threads may
 * stage packages at once; the devices of a multi-device context are staged in parallel).
 * A committee + bits set (LSG_PK_BITS) of n bits counts 16 + ceil(n / 32) toward max_pks; its
 * bit arena is reserved once the context has a committee registered (call lsg_reserve after
 * lsg_committees_set, or again).  A multi-committee set (LSG_PK_BITS_MULTI) of n bits over k
 * listed committees counts 16 + 2 k + ceil(n / 32): every part starts on its own arena word
 * (at most ceil(n / 32) + k words) and the plan holds 5 + 4 k words plus up to 32 lane pairs. */
int lsg_reserve(lsg_ctx* ctx, size_t max_sets, size_t max_pks, size_t max_msg_bytes, int32_t n_slots);
/* Device + pinned allocations made by this process so far (steady-state checks). */
int lsg_allocation_count(lsg_ctx* ctx, uint64_t* n);

/* worker.ts:30-106 for one work package (BlsWorkReq[] -> BlsWorkResult), asynchronous:
 * submit copies the jobs into pinned staging memory, draws the RLC randomizers, launches every
 * stage and returns a ticket (LSG_ERR_BUSY when all slots are outstanding: back-pressure as in
 * canAcceptWork, multithread/index.ts:143-149).  All batchable sets of the package form ONE
 * RLC group (one final exponentiation); only if it fails are the reference's 16-job chunks
 * and then the jobs of failing chunks checked (on the resident per-set values), so verdicts
 * and the batch_retries / batch_sigs_success counters are those of worker.ts.  wait blocks on
 * the ticket and applies those rules.  seed != 0 makes the randomizers deterministic (tests);
 * seed == 0 draws them from getrandom (LSG_ERR_ENTROPY if that fails).
 * A key that does not deserialize anywhere in the package (any device of the context) rejects
 * every job with the code of the first bad key in caller job order (worker.ts:41-43).
 * On a multi-device context the 16-job chunks are formed per device, so batch_retries /
 * batch_sigs_success can differ from a single device's; per-job verdicts never do.
 * A wait that fails before resolving (a device error while blocking) leaves the ticket
 * outstanding: it may be waited on again. */
int lsg_submit_jobs(lsg_ctx* ctx, const lsg_job* jobs, size_t n_jobs, uint64_t seed, lsg_ticket* ticket);
int lsg_wait_jobs(lsg_ctx* ctx, lsg_ticket ticket, lsg_job_result* results /* [n_jobs] */, lsg_stats* stats);
/* One process per GPU (SURVEY.md 8e over torch.distributed / any host collective), on a
 * single-device context: lsg_jobs_partial blocks until the package group's Miller product is
 * ready and writes it (576 bytes, canonical; the identity when the package has no batchable
 * set; *has_batch says which).  The caller all-gathers the partials, checks their product with
 * lsg_final_*, and resolves the ticket with that node verdict (1 passed, 0 failed: this GPU's
 * own package check then localises).  lsg_wait_jobs == lsg_wait_jobs_node(..., -1, ...).
 * The node verdict is advisory: this GPU's own check of its share is computed in any case and
 * decides, so a caller whose exchange went wrong (node_valid 1 but this share invalid) gets
 * the localised per-job verdicts, never a wrongly accepted package. */
int lsg_jobs_partial(lsg_ctx* ctx, lsg_ticket ticket, uint8_t* out576, int32_t* has_batch);
/* The same partial copied device-to-device into dev_out576 (576 bytes of device memory on the
 * context's device, e.g. the send buffer of an RCCL all-gather): the exchange never leaves the
 * GPU.  Returns once the copy is done. */
int lsg_jobs_partial_device(lsg_ctx* ctx, lsg_ticket ticket, void* dev_out576, int32_t* has_batch);
int lsg_wait_jobs_node(lsg_ctx* ctx, lsg_ticket ticket, int32_t node_valid, lsg_job_result* results,
                       lsg_stats* stats);
/* A package that also returns, per caller-named group, the compressed sum of the signatures of
 * the sets that verified: the op pools merge one 96-byte aggregate per
 * (package, key) instead of decoding and adding one signature per attestation
 * (opPools/attestationPool.ts:182-199).  lsg_set and lsg_job keep their layout; set_group has
 * one word per set, in job order and then set order.
 *   Values.  set_group[i] is below n_groups, or LSG_NO_GROUP for a set that joins no group.
 *     Any other value is a caller bug: LSG_ERR_INVALID_ARG before a slot is taken, and the
 *     context stays usable.  set_group == NULL or n_groups == 0 is exactly lsg_submit_jobs: it
 *     stages, allocates and launches what that call does.
 *   Included sets.  A set is included exactly when its job resolves to LSG_VALID: a multi-set
 *     job is all or nothing, as its verdict is; a package rejected by a key error includes
 *     nothing.
 *   Aggregate.  agg96[g] is the ZCash-compressed sum of the included signatures of group g
 *     (Signature.aggregate(sigs).toBytes()): the same point, hence the same bytes, as
 *     lsg_aggregate_signatures over those signatures.  A sum at infinity is 0xc0 || 0^95.
 *   Count.  agg_n[g] is how many signatures were summed.  With none included agg_n[g] = 0 and
 *     agg96[g] is 96 zero bytes.
 *   Duplicates.  A signature listed twice is added twice (the caller's business, as in
 *     Signature.aggregate).  96- and 192-byte signatures may share a group.
 *   Nothing else changes.  For a given seed, verdicts, error codes, their precedence, the batch
 *     counters, lsg_stats and the exported partial are those of the same package through
 *     lsg_submit_jobs.
 *   Mixing wait calls.  lsg_wait_jobs on a grouped ticket resolves it and drops the aggregates
 *     (as lsg_wait_jobs_grouped with agg96 or agg_n NULL does); lsg_wait_jobs_grouped on a plain
 *     ticket writes no aggregate; lsg_poll works.  lsg_wait_jobs_grouped is the node_valid = -1
 *     form only.
 *   Scope.  A grouped package launches on its own: it is never held by lsg_set_coalesce and
 *     does not flush what that holds, exactly as the packages of lsg_verify_deposits behave.
 *     On a context over several devices a submit with n_groups > 0 returns
 *     LSG_ERR_INVALID_ARG (a group can span devices; lsg_batch_partial and coalescing are
 *     single-device too).
 *   Allocation.  The per-slot buffers (group ids, gather list and chunk plan, projective sums,
 *     96 * n_groups bytes of output) are allocated by the first grouped package.  lsg_reserve
 *     sizes them for max_sets sets and max_sets groups once the context has seen a grouped
 *     submit: the caller reserves again after that (the committee bit arena's rule), and a
 *     reserved context within those bounds then allocates nothing.  A context that never groups
 *     allocates what it did before. */
#define LSG_NO_GROUP 0xffffffffu
int lsg_submit_jobs_grouped(lsg_ctx* ctx, const lsg_job* jobs, size_t n_jobs, uint64_t seed,
                            const uint32_t* set_group, size_t n_groups, lsg_ticket* ticket);
int lsg_wait_jobs_grouped(lsg_ctx* ctx, lsg_ticket ticket, lsg_job_result* results, lsg_stats* stats,
                          uint8_t* agg96 /* n_groups x 96 */, uint32_t* agg_n /* n_groups */);
/* Coalescing of small packages (single-device contexts; off by default).  From this call on,
 * a package of at most max_sets sets submitted with lsg_submit_jobs is copied (the caller's
 * buffers are free on return) and, while max_inflight launches are on the device, held back;
 * the held packages go out together as ONE launch when the device has room (a wait frees a
 * slot) or when one of them is waited on.  Every package keeps the reference's semantics on
 * its own (multithread/index.ts:335 one package per worker; worker.ts:30-106): its
 * batchable jobs in 16-job chunks each checked as one RLC batch, per-job retry, the
 * deserializeSet rule over its jobs, its own counters (n_final_exps counts the whole launch).
 * Such tickets have no node protocol: lsg_jobs_partial* and lsg_wait_jobs_node with
 * node_valid != -1 reject them.  This fills the GPU with many small packages (gossip-sized)
 * without one launch -- and one chain of dependent kernels -- per package.  max_sets = 0 turns
 * coalescing off (held packages are launched first). */
int lsg_set_coalesce(lsg_ctx* ctx, uint32_t max_sets, int32_t max_inflight);
/* Whole-job assignment of lsg_init_devices (host only, no device needed): owner[j] = device of
 * job j = floor(sets before j * n_devices / total sets). */
int lsg_assign_jobs(const uint32_t* job_sets, size_t n_jobs, int32_t n_devices, int32_t* owner);
/* Number of pipeline slots (packages that may be outstanding at once): the back-pressure
 * bound of canAcceptWork (multithread/index.ts:143-149 workersBusy < poolSize). */
int lsg_pipeline_slots(lsg_ctx* ctx, int32_t* n);
/* *done = 1 once the ticket's device work has finished (any ticket kind). */
int lsg_poll(lsg_ctx* ctx, lsg_ticket ticket, int32_t* done);
/* submit + wait */
int lsg_verify_jobs(lsg_ctx* ctx, const lsg_job* jobs, size_t n_jobs, uint64_t seed, lsg_job_result* results,
                    lsg_stats* stats);

/* maybeBatch.ts:16-39 over one list of sets (no retry): *result = one lsg_job_result. */
int lsg_verify_sets(lsg_ctx* ctx, const lsg_set* sets, size_t n_sets, uint64_t seed, lsg_job_result* result);

/* PublicKey.aggregate(pks).toBytes(uncompressed): out96 receives the 96-byte affine sum.
 * *err_code = BLST_* for a bad input key, LSG_ERR_EMPTY_AGGREGATE for n == 0.  With
 * pk_len == LSG_PK_INDEX, pks holds n uint32 indices into the pubkey table. */
int lsg_aggregate_pubkeys(lsg_ctx* ctx, const uint8_t* pks, uint32_t pk_len, size_t n, uint8_t* out96,
                          int32_t* err_code);
/* PublicKey.aggregate for n_sets sets in one device pass (utils.ts:11 getAggregatedPubkey over
 * a block's aggregate sets, indexedAttestation.ts:21-47): set i's keys are sets[i].pks /
 * pk_len / n_pks (bytes, table indices, a committee id + bits, or a committee list + bits
 * (LSG_PK_BITS_MULTI: k_pk_agg_bits_multi); msg and sig are ignored).  out96[96 i..] = set i's
 * uncompressed sum; err[i] = its first bad key's BLST_* / LSG_ERR_BAD_INDEX, or
 * LSG_ERR_EMPTY_AGGREGATE for no keys, LSG_ERR_BAD_COMMITTEE for a LSG_PK_BITS set naming no
 * registered committee of its length.  Every input size runs the jobs path's fused gather +
 * mixed-addition fold (k_pk_agg_seg; LSG_PK_BITS sets: k_pk_agg_bits); the batch-affine aggregation tree exists only in the
 * A/B build (liblodestar_bls_ab.so, LSG_AGG_TREE=1), where it was measured slower. */
int lsg_aggregate_pubkeys_multi(lsg_ctx* ctx, const lsg_set* sets, size_t n_sets, uint8_t* out96, int32_t* err);

/* hash_to_G2(msg_i, DST) for n messages of msg_len bytes each -> n x 192-byte uncompressed points. */
int lsg_hash_to_g2(lsg_ctx* ctx, const uint8_t* msgs, uint32_t msg_len, size_t n, const uint8_t* dst,
                   uint32_t dst_len, uint8_t* out192);

/* Signature.fromBytes(sig, affine, validate=true) for n signatures of sig_len bytes:
 * out192[i] = uncompressed affine point, err[i] = BLST_* (0 = ok). */
int lsg_sig_decode(lsg_ctx* ctx, const uint8_t* sigs, uint32_t sig_len, size_t n, uint8_t* out192, int32_t* err);

/* One shard's sets -> its un-exponentiated Miller product (576 bytes: 12 canonical big-endian
 * Fp in tower order) over the sets that decode, and per-set error codes (synchronous;
 * single-device contexts).  *any_error != 0 means the shard cannot be batched as a whole. */
int lsg_batch_partial(lsg_ctx* ctx, const lsg_set* sets, size_t n_sets, uint64_t seed, uint8_t* out576,
                      int32_t* set_err, int32_t* any_error);
/* prod(partials) -> final exponentiation on the GPU -> *valid = (result == 1).  The
 * submit/wait pair runs on device 0's final-exponentiation entries, overlapping packages. */
int lsg_final_verify(lsg_ctx* ctx, const uint8_t* partials576, size_t n_partials, int32_t* valid);
int lsg_final_submit(lsg_ctx* ctx, const uint8_t* partials576, size_t n_partials, lsg_ticket* ticket);
/* lsg_final_submit over partials in device memory of device 0 (an all-gather's output); the
 * caller's writes to them must be complete (e.g. its stream synchronised). */
int lsg_final_submit_device(lsg_ctx* ctx, const void* dev_partials576, size_t n_partials, lsg_ticket* ticket);
int lsg_final_wait(lsg_ctx* ctx, lsg_ticket ticket, int32_t* valid);
/* Several RLC batches' final checks in one ticket (one launch per stage instead of one
 * ticket per batch): n_groups groups of per_group partials each, group g being partials
 * g*per_group .. g*per_group+per_group-1 (e.g. one per rank); lsg_final_wait_groups writes
 * n_groups verdicts.  lsg_final_submit(p, n) is lsg_final_submit_groups(p, 1, n). */
int lsg_final_submit_groups(lsg_ctx* ctx, const uint8_t* partials576, size_t n_groups, size_t per_group,
                            lsg_ticket* ticket);
int lsg_final_wait_groups(lsg_ctx* ctx, lsg_ticket ticket, int32_t* valid /* [n_groups] */);

/* ---- Validator pubkey table resident in HBM.  Replaces the per-call
 * PublicKey -> bytes hand-off of the pool (multithread/index.ts:177, utils.ts:11) with the
 * node's index2pubkey cache held on the GPU (state-transition/src/cache/pubkeyCache.ts:60-75
 * syncPubkeys, cache/epochContext.ts:701-704 addPubkey): keys are decoded once, as
 * PublicKey.fromBytes(pk, jacobian) does there (on-curve check, no subgroup check: cached
 * keys were validated at deposit time), and sets then name their keys by index
 * (lsg_set.pk_len = LSG_PK_INDEX); aggregation gathers them on the device.
 *   lsg_pubkey_table_set  keys first_index .. first_index+n-1 <- pks (48 or 96 bytes each);
 *                         the table grows as needed (growth waits for in-flight work).
 *                         err[k] (may be NULL) = BLST_* of key k; a key that does not decode
 *                         leaves its index unset, and a set naming an unset index fails
 *                         its package with LSG_ERR_BAD_INDEX (as deserializeSet throws).
 *   lsg_pubkey_table_size number of indices (highest set index + 1). */
int lsg_pubkey_table_set(lsg_ctx* ctx, size_t first_index, const uint8_t* pks, uint32_t pk_len, size_t n,
                         int32_t* err);
int lsg_pubkey_table_size(lsg_ctx* ctx, size_t* n);

/* ---- Committees resident on the GPU.  An attestation or a sync aggregate
 * reaches the node as a committee plus a bitfield (aggregationBits.intersectValues(committee),
 * state-transition/src/cache/epochContext.ts:620-623; syncCommitteeBits.intersectValues,
 * block/processSyncCommittee.ts:87-90), and committees are fixed for an epoch.  With the
 * committees held beside the pubkey table a set names its keys as committee id + bits
 * (lsg_set.pk_len = LSG_PK_BITS, ~60 bytes instead of ~1.8 KB of indices), and its aggregate
 * is the cheaper of  sum of the participants  and  committee sum - sum of the absentees  --
 * the same point, so verdicts and serialised aggregates are those of the index form.
 *   lsg_committees_set    committee first_id + c <- members indices[offsets[c] .. offsets[c+1])
 *                         (rows of the pubkey table; duplicates allowed, as a sync committee has
 *                         them; offsets has n_committees + 1 entries, offsets[0] = 0).  One
 *                         device pass over all of them stores the index rows and each full sum
 *                         (projective; a row holding the infinity key adds nothing) on every
 *                         device.  err[c] (may be NULL) = LSG_ERR_BAD_INDEX when a member names
 *                         an unset row, LSG_ERR_EMPTY_AGGREGATE for an empty committee; such a
 *                         committee stays unset.  ids are below 2^20 and a committee has at most
 *                         131,072 members (else LSG_ERR_INVALID_ARG).  Registering an id again
 *                         replaces it.  Waits for in-flight work, as a table rewrite does.
 *                         A lsg_pubkey_table_set call that writes a row below the current table
 *                         size (a rewrite, not an append) unsets EVERY committee -- a stored
 *                         sum may be stale -- and they are registered again.
 *   lsg_committees_clear  unsets ids first_id .. first_id + n - 1.
 *   lsg_committee_count   highest set id + 1.
 * A context that never registers a committee behaves, allocates and launches as before. */
int lsg_committees_set(lsg_ctx* ctx, uint32_t first_id, const uint32_t* indices,
                       const uint32_t* offsets /* n_committees + 1, offsets[0] = 0 */, size_t n_committees,
                       int32_t* err /* may be NULL */);
int lsg_committees_clear(lsg_ctx* ctx, uint32_t first_id, size_t n);
int lsg_committee_count(lsg_ctx* ctx, size_t* n);

/* The message cache: an opt-in, per-device cache of the affine G2 points H(m)
 * under the POP DST, kept across packages.  A slot's 64 AttestationData are signed by tens of
 * thousands of attesters whose sets arrive spread over hundreds of gossip-sized packages; with
 * the cache on, a message the device hashed for an earlier package is not staged, not copied
 * to the device and not hashed again (nor is its signing root computed, when it is an
 * LSG_MSG_OBJECT message).
 *   lsg_msg_cache_set(capacity)  allocates `capacity` rows per device (0: off, everything freed)
 *                                and the host key store; waits for the work in flight and
 *                                drops every entry, as does lsg_msg_cache_clear.  Call
 *                                lsg_reserve after it (or again): it sizes the per-slot
 *                                buffers of cached packages, which then allocate nothing.
 *   lsg_msg_cache_get_stats      counters summed over the devices.
 * The key is the message as it is staged -- payload bytes plus the LSG_MSG_OBJECT marker of
 * its length -- compared on every byte; empty messages and messages of more than 192 bytes
 * are never cached (`bypassed`).  The package that first sees a message hashes it and writes
 * the point into a row; the entry becomes visible once the host has observed that launch's
 * completion (lsg_wait_jobs*, lsg_poll).  Until then other packages naming the message hash it
 * themselves (`pending`).  Rows a launch reads or writes are pinned until then; with every row
 * pinned a new message is hashed and not inserted (`full`).  Replacement is CLOCK with a
 * second chance for rows that were hit.  lookups == hits + pending + inserts + full.
 * The cache serves the packages of lsg_submit_jobs* / lsg_verify_jobs / lsg_verify_sets on
 * every device of the context (each device keeps its own); lsg_hash_to_g2 (caller's DST),
 * lsg_verify_deposits on one device (its messages stay on the device) and lsg_batch_partial do
 * not use it.  Verdicts, error codes, counters, aggregates and exported partials are those of
 * a context without the cache: a stored point is the computed point copied word for word.
 * A context that never calls lsg_msg_cache_set stages, allocates and launches as before. */
typedef struct {
  uint64_t lookups, hits, pending, inserts, evictions, bypassed, full;
  uint32_t entries, capacity;
} lsg_msg_cache_stats;
int lsg_msg_cache_set(lsg_ctx* ctx, size_t capacity);
int lsg_msg_cache_clear(lsg_ctx* ctx);
int lsg_msg_cache_get_stats(lsg_ctx* ctx, lsg_msg_cache_stats* out);

/* Batched KeyValidate: PublicKey.fromBytes(pk, affine, validate=true) of
 * processDeposit.ts:57-65 for n keys of pk_len (48/96) bytes -- decode, not the point at
 * infinity (BLST_PK_IS_INFINITY), in the r-torsion subgroup (BLST_POINT_NOT_IN_GROUP).
 * err[i] = BLST_* (0 = valid); out96 (may be NULL) = the uncompressed affine key. */
int lsg_pubkey_validate(lsg_ctx* ctx, const uint8_t* pks, uint32_t pk_len, size_t n, uint8_t* out96, int32_t* err);

/* G2 signature aggregation for the op pools:
 *   bls.Signature.aggregate(sigs.map(signatureFromBytesNoCheck)).toBytes()
 * of opPools/attestationPool.ts:195, syncCommitteeMessagePool.ts:139,
 * aggregatedAttestationPool.ts:322 and syncContributionAndProofPool.ts:185, with the decode of
 * opPools/utils.ts:32-34 (Signature.fromBytes(sig, affine, validate=false): size, encoding and
 * on-curve checks, no subgroup check).  n_groups independent aggregations in one call: group g
 * is signatures offsets[g] .. offsets[g+1]-1 (offsets has n_groups+1 entries, offsets[0] = 0),
 * each sig_len (96 or 192) bytes.  out96[g] = the compressed sum (zeros unless err[g] == 0);
 * err[g] = BLST_* of the group's first signature that does not decode, or
 * LSG_ERR_EMPTY_AGGREGATE for an empty group ("EMPTY_AGGREGATE_ARRAY"). */
int lsg_aggregate_signatures(lsg_ctx* ctx, const uint8_t* sigs, uint32_t sig_len, const uint32_t* offsets,
                             size_t n_groups, uint8_t* out96, int32_t* err);

/* Signing roots on the GPU: computeSigningRoot(type, obj, domain) of
 * state-transition/src/util/signingRoot.ts:7-13 = hash_tree_root(SigningData{objectRoot, domain}).
 *   lsg_signing_roots              objectRoot given: roots32 = n x 32 bytes;
 *   lsg_attestation_signing_roots  getAttestationDataSigningRoot (signatureSets/indexedAttestation.ts:11-19):
 *                                  data128 = n SSZ-serialized phase0.AttestationData (128 bytes each:
 *                                  slot, index, beaconBlockRoot, source{epoch, root}, target{epoch, root}).
 * domain_stride 0: one 32-byte domain for every object; 32: one per object.  out32 = n x 32 bytes,
 * the 32-byte messages lsg_set.msg carries. */
int lsg_signing_roots(lsg_ctx* ctx, const uint8_t* roots32, size_t n, const uint8_t* domain32, uint32_t domain_stride,
                      uint8_t* out32);
int lsg_attestation_signing_roots(lsg_ctx* ctx, const uint8_t* data128, size_t n, const uint8_t* domain32,
                                  uint32_t domain_stride, uint8_t* out32);
/* The deposit kind (block/processDeposit.ts:49-54 computeSigningRoot(ssz.phase0.DepositMessage, ..)):
 * msgs88 = n SSZ-serialized DepositMessage (88 bytes each: pubkey 48, withdrawalCredentials 32,
 * amount u64 little-endian).  The caller supplies the domain: computeDomain(DOMAIN_DEPOSIT,
 * GENESIS_FORK_VERSION, ZERO_HASH) is one constant per network. */
int lsg_deposit_signing_roots(lsg_ctx* ctx, const uint8_t* msgs88, size_t n, const uint8_t* domain32,
                              uint32_t domain_stride, uint8_t* out32);
/* Any tag-0 object kind of LSG_MSG_OBJECT by its serialized length: objs = n objects of obj_len
 * bytes each, obj_len one of 8, 16, 32, 76, 88, 112, 128, 264 (another length: LSG_ERR_INVALID_ARG).  The
 * roots are those a package computes for marked sets (one dispatcher, lsg_ssz.hpp); for 32, 128
 * and 88 they equal the three calls above. */
int lsg_object_signing_roots(lsg_ctx* ctx, const uint8_t* objs, uint32_t obj_len, size_t n, const uint8_t* domain32,
                             uint32_t domain_stride, uint8_t* out32);
/* The variable-size kinds: n objects of one kind tag (LSG_MSG_KIND_AGG_PROOF*), object i the bytes
 * objs[offsets[i] .. offsets[i + 1]) (offsets: n + 1 entries, offsets[0] = 0).  Runs k_msg_roots_var,
 * the kernel a package runs for tagged sets.  Kind 0, an unknown kind or a malformed object:
 * LSG_ERR_INVALID_ARG. */
int lsg_object_signing_roots_var(lsg_ctx* ctx, uint32_t kind, const uint8_t* objs, const uint32_t* offsets, size_t n,
                                 const uint8_t* domain32, uint32_t domain_stride, uint8_t* out32);

/* processDeposit.ts:47-66 for n deposits in one device pass, synchronous, any n.  data184 = n
 * SSZ-serialized DepositData (184 bytes each: pubkey 48, withdrawalCredentials 32, amount u64,
 * signature 96).  valid[i] = 1 exactly when the reference would go on to add the validator:
 * PublicKey.fromBytes(pubkey, affine, true), Signature.fromBytes(sig, affine, true) and verify
 * over the DepositMessage signing root all pass.  err[i] = 0 when key and signature both passed
 * validation (whether or not the signature then verified), else the BLST_* code of the first
 * failing step: key, then signature.  The signing roots are computed on the device and (on a
 * single-device context) stay there as the messages; each deposit is one single-set batchable
 * job with LSG_JOB_VALIDATE_KEYS, run through the package machinery -- one RLC check first,
 * then the chunk and per-job fallback -- in packages of at most 8,192 deposits, up to four of
 * them outstanding on free pipeline slots (LSG_ERR_BUSY only when other tickets hold
 * every slot; valid and err are then incomplete and the caller repeats the call, as it would
 * lsg_submit_jobs).  The packages launch on
 * their own: they are never held by lsg_set_coalesce and do not flush what it holds, so packages
 * held for coalescing go out when their own rules say, possibly behind the deposits' slots.
 * seed as in lsg_submit_jobs.  Calls are serialised among themselves. */
int lsg_verify_deposits(lsg_ctx* ctx, const uint8_t* data184, size_t n, const uint8_t* domain32, uint64_t seed,
                        uint8_t* valid, int32_t* err);

/* Test/bench input generation (not on the verify path): sig_i = sk_i * H(m_i) compressed,
 * pk_i = sk_i * G1 uncompressed; sks are 32-byte big-endian secret keys. */
int lsg_sign(lsg_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs, uint32_t msg_len, size_t n, uint8_t* out96);
int lsg_sk_to_pk(lsg_ctx* ctx, const uint8_t* sks32, size_t n, uint8_t* out96);

/* Parity hook of the device Fp2 product (tests only): for n items of four field elements
 * (a0, a1, b0, b1) in the pair layout -- 14 signed radix-2^29 limbs each, word k of element e
 * of item i at in[(4 i + e) * 14 + 2 (k mod 7) + k / 7] -- writes c0, c1 with
 * c0 + c1 u = (a0 + a1 u)(b0 + b1 u) / 2^406 mod p, raw (lazy, not canonical), same layout, 2
 * elements per item.  Not on the verification path. */
int lsg_check_fp2_mul(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
/* Parity hooks of the device squaring leaves (tests only), same layout and raw outputs:
 * lsg_check_fp_sqr takes one element a per item (14 words) and writes a^2 / 2^406 mod p (14
 * words); lsg_check_fp2_sqr takes (a0, a1) (28 words) and writes c0, c1 with
 * c0 + c1 u = (a0 + a1 u)^2 / 2^406 mod p (28 words).  Not on the verification path. */
int lsg_check_fp_sqr(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
int lsg_check_fp2_sqr(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
/* Parity hook of the lazy sums (tests only), same layout and raw outputs: 12 elements per item
 * in (the 12 n elements form a ring; item i works on the elements from 12 i on), 42 per item
 * out: the maximal admissible sum, the small multiples, fp2_mul_b3, jac_dbl over Fp and Fp2,
 * the G2 addition and one combination of the fused Miller kernel, each with the form that
 * carries at every operation beside it (lsg_k_reduce.hip k_check_sums lists the slots).  Not
 * on the verification path. */
int lsg_check_sums(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
/* Parity hooks of the Fp2 layout with one component per lane (the [x] chains of k_sig_subgroup
 * and k_h2c_clear; tests only, not on the verification path).  Elements travel in the pair
 * layout above, raw in and raw out; Fp2 value X_j of an item is its elements (2 j, 2 j + 1).
 *
 * lsg_check_fp2_lanes: 12 elements per item in (A, B, C, D, E, F = X_0 .. X_5), 24 per item out.
 * Y_j = out elements (24 i + 2 j, 24 i + 2 j + 1), converted back to the pair layout:
 *    Y_0  A through the conversion in and out (the same words)
 *    Y_1  A B / 2^406          Y_2  A^2 / 2^406         (mod p, the leaves' normalised limbs)
 *    Y_3  (A + B + C - D - E - F) carried once
 *    Y_4 .. Y_8  2A, 3A, 4A, 8A, 12A (carry_mul)
 *    Y_9  12 (1 + u) A         Y_10  -A
 * and out words (24 i + 22) * 14 .. + 27: A as the lanes hold it, word k of lane h (0: even, 1:
 * odd lane of the item's pair) at 2 k + h -- limb k of c0 on lane 0, of c1 on lane 1.
 *
 * lsg_check_g2_lanes: 12 elements per item in: a Jacobian point J = (X_0, X_1, X_2) and a
 * homogeneous point Q = (X_3, X_4, X_5); 24 per item out: jac_dbl(J) computed in the lane
 * layout (Y_0 .. Y_2), in the pair layout (Y_3 .. Y_5), jac_add_proj(J, Q) in the lane layout
 * (Y_6 .. Y_8), in the pair layout (Y_9 .. Y_11). */
int lsg_check_fp2_lanes(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
int lsg_check_g2_lanes(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
/* lsg_check_mf_lanes: the pieces of the layout that only the fused Miller kernel uses; 12 elements
 * per item in (A .. F as for lsg_check_fp2_lanes, D .. F unused), 24 out, every lane-layout result
 * converted back and followed by the pair form's: Y_0 = A B.c0 (Fp2 x Fp), Y_1 its pair-form twin;
 * Y_2, Y_3 = xi A carried; Y_4, Y_5 = A + xi (B - C) with one carry; Y_6 .. Y_8 = v (A, B, C) =
 * (xi C, A, B); Y_9 = 1, Y_10 = 0; elements 22, 23: B.c0 spread over both lanes as they hold it
 * (word k of lane h at 2 k + h). */
int lsg_check_mf_lanes(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
/* lsg_check_pow_lanes: the fixed-exponent power kernel with one Fp element per lane
 * (k_fp_pow_lanes: the square roots of the signature decode and the SSWU map in large launches)
 * on the caller's limb words: n raw elements in the pair layout in, out[i] = in[i]^e / R^(e-1)
 * raw, for id 0: e = p - 2, 1: (p + 1) / 4, 2: (p - 3) / 4.  lsg_check_pow_pair: the pair form's
 * power (pair_pow_plan, what the single kernels run) on the same words; the two agree word for
 * word.  LSG_ERR_INVALID_ARG for another id.  Tests only. */
int lsg_check_pow_lanes(lsg_ctx* ctx, int32_t id, const uint32_t* in, size_t n, uint32_t* out);
int lsg_check_pow_pair(lsg_ctx* ctx, int32_t id, const uint32_t* in, size_t n, uint32_t* out);
/* lsg_check_msm_buckets: the bucket pass of the signature MSM on the caller's points, flags, index
 * list and chunk triples.  sigs96: n compressed G2 points, decoded without the subgroup check
 * (every one must decode); err / inf / pinf: the n per-point flags the pass sees in place of the
 * decode's own (a point with any of them set adds nothing); idx: the list of n_idx point numbers;
 * chunks: n_chunks triples {off, len, out} of the first pass, 2^ips_log2 lane pairs each
 * (ips_log2 <= 5), summing idx[off .. off + len) into output `out` >= 0 or into partial sum
 * -out - 1 < n_tmp; chunks2 (n_chunks2 may be 0): the triples of a second pass over the partial
 * sums off .. off + len, outputs only.  Every partial sum and every one of the n_out outputs must
 * be written exactly once.  mode 0: k_msm_bucket_seg (the fold with one Fp2 component per lane),
 * 1: its pair-form twin, 2: projective copies (k_sig_proj) summed by k_seg_reduce<1>.  out96: the
 * n_out sums, compressed (projective representatives differ between the modes).
 * LSG_ERR_INVALID_ARG for anything out of range.  Tests only. */
int lsg_check_msm_buckets(lsg_ctx* ctx, int32_t mode, const uint8_t* sigs96, size_t n, const int32_t* err,
                          const uint8_t* inf, const uint8_t* pinf, const int32_t* idx, size_t n_idx,
                          const int32_t* chunks, size_t n_chunks, int32_t ips_log2, const int32_t* chunks2,
                          size_t n_chunks2, int32_t ips_log2_2, size_t n_tmp, size_t n_out, uint8_t* out96);
/* Parity hooks of the layer between the products and the accept / reject rules (tests only;
 * none is on the verification path).  Elements travel in the pair layout above: 14 words, limb
 * L at word 2 (L mod 7) + L / 7.  Each returns LSG_ERR_INVALID_ARG for a null pointer with a
 * non-zero count or a count whose buffers pass 2^31 bytes.
 *
 * lsg_check_canon: n raw lazy elements in (element i at in[14 i ..]), 54 words per element out:
 *    out[54 i +  0 .. 13]  pair_canon(a): the representative in [0, p) of any lazy value
 *    out[54 i + 14 .. 27]  fp_canonical(a): the same for a value in (-p, 2p)
 *    out[54 i + 28 .. 39]  the 48 bytes fp_to_be48(fp_canonical(a)) writes, in memory order
 *    out[54 i + 40]        bit 0 fp_is_zero(a), bit 1 fp_canon_lt_p(a), bit 2 fp_canon_gt_half(a),
 *                          bit 3 fp_canon_parity(a)
 *    out[54 i + 41]        0
 *    out[54 i + 42 .. 53]  the 48 bytes fp_to_be48(a) writes for the raw value (a in [0, 2^384):
 *                          the form that carries the flag bits 381..383)
 * and, for nb big-endian 48-byte strings at bytes48, fp_from_be_bytes(b, 12) as 14 words per
 * string in out_limbs.  Either count may be 0 (its pointers are then not read).
 *
 * lsg_check_fp2_roots: n Fp2 elements (a0, a1) in Montgomery form, lazy limbs allowed
 * (in[28 i ..] = a0, in[28 i + 14 ..] = a1), 58 words per item out, field values raw:
 *    out[58 i +  0 .. 27]  the root fp2_sqrt leaves, (c0, c1) (a square root when bit 0 is set)
 *    out[58 i + 28 .. 41]  fp_inv(a0), the fixed-exponent power
 *    out[58 i + 42 .. 55]  pair_mont_mul(pair_inv_gcd(pair_canon(a0)), R^3): the divstep
 *                          inversion as the batched inversions' roots run it
 *    out[58 i + 56]        bit 0 fp2_sqrt's result, bit 1 fp2_sgn0(a), bit 2 fp2_lexi_largest(a),
 *                          bit 3 fp2_is_zero(a)
 *    out[58 i + 57]        0
 * Both inverses x of a0 satisfy x a0 = 2^812 (mod p) as integers, and x = 0 (mod p) for a0 = 0.
 *
 * lsg_check_batch_inv: n raw elements in (14 words each), the n outputs of the host's batched
 * inversion of them (the call the hash and key stages make) out, raw, same congruence; zeros
 * in any representation come out as zero.
 *
 * lsg_check_map_uniform: lsg_hash_to_g2 from the expanded messages on: n x 256 caller-chosen
 * "uniform bytes" (four 64-byte big-endian integers per item: u0.c0, u0.c1, u1.c0, u1.c1) take
 * the place of expand_message_xmd's output; out192 receives the 192-byte uncompressed points
 * (the infinity encoding where the sum of the two mapped points is the identity). */
int lsg_check_canon(lsg_ctx* ctx, const uint32_t* in, size_t n, const uint8_t* bytes48, size_t nb, uint32_t* out,
                    uint32_t* out_limbs);
int lsg_check_fp2_roots(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
int lsg_check_batch_inv(lsg_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out);
int lsg_check_map_uniform(lsg_ctx* ctx, const uint8_t* ub256, size_t n, uint8_t* out192);
/* Parity hook of the random linear combination (tests only): lsg_batch_partial in every respect
 * -- one batchable job, every set scaled, the same slot, plan, kernels and launches, per-set
 * error codes, single-device contexts -- except that set i takes the randomizer rnd[i] where
 * lsg_batch_partial takes the i-th draw of its seed, so that a test can put edge scalars, equal
 * scalars and skewed bucket occupancies through the scaling kernels and the bucket sums.  The
 * pointer travels with the call (no context state: concurrent submitters are unaffected).
 * LSG_ERR_INVALID_ARG, before anything is staged, for a null pointer (set_err may be null), a zero
 * randomizer or a multi-device context; the context stays usable.  It adds no power to the
 * library: a nonzero seed already fixes every randomizer. */
int lsg_check_batch_partial_rnd(lsg_ctx* ctx, const lsg_set* sets, size_t n_sets,
                                const uint64_t* rnd /* [n_sets], each nonzero */, uint8_t* out576,
                                int32_t* set_err, int32_t* any_error);

/* Integer-VALU roofline probe: runs a throughput kernel of dependent-free 381-bit
 * Montgomery multiplications; reports Fp-mul/s and v_mad_u64_u32/s (x300 per mul). */
int lsg_probe_fp_mul_rate(lsg_ctx* ctx, double* fp_mul_per_s, double* mad_per_s);

/* Integer-VALU peak probe: issue rate of v_mad_u64_u32 (16 independent accumulators per lane,
 * 8 waves per SIMD) -- the roofline denominator bench.py reports. */
int lsg_probe_mad_peak(lsg_ctx* ctx, double* mad_per_s);

/* Per-kernel timing of the most recently completed ticket (or synchronous call), from HIP
 * events on the streams the kernels ran on: names[i] / ms[i] for up to max entries;
 * returns the count. */
int lsg_last_kernel_times(lsg_ctx* ctx, const char** names, double* ms, int max);

#ifdef __cplusplus
}
#endif
#endif /* LODESTAR_BLS_H */
