// lsg_host.hip -- host orchestration and the C ABI (include/lodestar_bls.h) of the MI355X
// BLS12-381 signature-set verifier.  No kernels live here (they are in lsg_k_*.hip and
// lsg_slp.hip, reached through lsg_launch.h / lsg_slp.h).
//
// Reference path replaced (file:line under /root/reference):
//   packages/beacon-node/src/chain/bls/multithread/worker.ts:30-114  verifyManySignatureSets,
//       deserializeSet: batch-of-jobs verification with the per-job retry fallback
//   packages/beacon-node/src/chain/bls/maybeBatch.ts:16-39         RLC batch vs single verify
//   packages/beacon-node/src/chain/bls/utils.ts:5-26               pubkey aggregation
//   + the un-vendored @chainsafe/blst@0.2.8 arithmetic underneath.
//
// One package (BlsWorkReq[]: the jobs one worker would get) runs as ONE ticket:
//   phase A (submit, no host synchronisation): every batchable set of the package is one RLC
//     group (bucket MSM for its signature sum), every non-batchable job its own group; each
//     group gets its Miller product and one final exponentiation, launched speculatively.
//   resolve (wait): the reference's verdict rules (worker.ts:51-96).  A passing package
//     group answers every batchable job at once; only when it fails are the 16-job chunks of
//     worker.ts (phase B) and then the jobs of failing chunks (phase C) checked, on the
//     per-set values still resident, so per-job verdicts and the batch_retries /
//     batch_sigs_success counters are the reference's.
// Which file holds what: this one has the device side -- streams, events, buffers, copies,
// kernel launches, tickets, locks.  The policy over small integers is host-only code in
// lsg_plan.hpp (namespace lsgp), tested on the CPU by tests/native/plancheck.cpp: the staging
// order and 16-job chunks of a package (PkgShape), its phase-A groups (plan_groups), the
// Miller items and segmented reductions of a phase (plan_phase, plan_seg), the KeyValidate and
// per-message lists (plan_validate_keys, plan_msg_lists), the deserializeSet rule
// (first_key_error) and the verdict rules (resolve_package, which calls back into
// run_fallback_phase here for every phase B0 / B / C1 / C2 it needs).  How the caller's sets
// become the staged bytes is host-only too, lsg_stage.hpp, tested by tests/native/stagecheck.cpp:
// the staging arena's layout (the one statement of its size), the distinct-message table, the
// message-cache decisions, committee and key-slot staging, the randomizers; stage_sets here
// sizes the buffers between its measuring and filling pass and issues the copies.
// Per device a context owns LSG_SLOTS pipeline slots (two streams each, all buffers
// preallocated by lsg_reserve); several devices share one ticket (whole jobs per device, one
// all-gather of the 576-byte partials, one node final exponentiation: SURVEY.md 8e).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <errno.h>
#include <string.h>
#include <sys/random.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../include/lodestar_bls.h"
#include "lsg_launch.h"
#include "lsg_layout.h"
#include "lsg_slp.h"
#include "lsg_ab.h"
#include "lsg_msg_cache.hpp"
#include "lsg_plan.hpp"
#include "lsg_stage.hpp"

using namespace lsgl;
using namespace lsgp;
static_assert(lsgp::MC_ROW == LSG_MC_ROW, "the stager's row marker is the one the kernels read");

namespace {

const uint8_t DST_POP[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
const uint32_t DST_POP_LEN = 43;
constexpr int LSG_SLOTS = 64;      // packages in flight per device (created on first use)
#ifndef LSG_DEFAULT_HW_QUEUES
#define LSG_DEFAULT_HW_QUEUES "16"  // GPU_MAX_HW_QUEUES when the process sets none (lsg_init_devices)
#endif
constexpr int LSG_FINALS = 64;     // final-exponentiation entries in flight (lsg_final_*)
constexpr int LSG_FE_STREAMS = 8;  // streams the final-exponentiation entries share
constexpr int LSG_MAX_DEVICES = 16;
constexpr int LSG_MILLER_KMAX = 4;

uint64_t now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);  // process.hrtime's clock (the Node host's metrics)
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// OS CSPRNG bytes (getrandom(2)); false if the kernel cannot provide them.  There is no
// deterministic fallback: predictable RLC multipliers would let forged sets cancel.
bool os_random(void* buf, size_t len) {
  uint8_t* p = (uint8_t*)buf;
  while (len) {
    ssize_t r = getrandom(p, len, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    p += r;
    len -= (size_t)r;
  }
  return true;
}

std::atomic<uint64_t> g_allocs{0};  // device + pinned allocations made (lsg_allocation_count)

// env LSG_TRACE_HOST=1: one stderr line per phase-A submission with its host time per stage
// (staging, planning, per-set launches, group launches), to find host-bound workloads
bool trace_host() {
  static const bool on = [] {
    const char* e = getenv("LSG_TRACE_HOST");
    return e && e[0] == '1';
  }();
  return on;
}

// env LSG_TRACE_ALLOC=1: one stderr line per allocation (size and caller), for steady-state checks
void trace_alloc(const char* kind, size_t bytes) {
  const char* e = getenv("LSG_TRACE_ALLOC");  // read per allocation: allocations are rare
  const bool on = e && atoi(e) != 0;
  if (on) fprintf(stderr, "[lsg alloc] %s %zu bytes\n", kind, bytes);
  (void)on;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
struct HostBuf {  // pinned host memory (async copies)
  void* p = nullptr;
  size_t cap = 0;
};
struct Timer {
  const char* name;
  hipEvent_t a, b;
};

}  // namespace

// ---------------------------------------------------------------------------- state
namespace {

enum SlotKind {
  SLOT_FREE = 0,
  SLOT_JOBS = 1,
  SLOT_STAGING = 2, /* reserved by a submission staging it with the context lock released */
  SLOT_FINAL = 3,
  SLOT_MERGE = 4 /* tickets of coalesced packages */
};

// a small package held for a coalesced launch (lsg_set_coalesce): the caller's jobs, sets
// and bytes copied, so the caller's buffers are free once lsg_submit_jobs returns
struct PendingPkg {
  uint64_t serial = 0, seed = 0;
  size_t n_sets = 0;
  std::vector<lsg_job> jobs;
  std::vector<lsg_set> sets;
  std::vector<uint8_t> data;
};
struct MergeTicket {
  int slot = -1;  // -1: not launched yet
  int sub = -1;
  int rc = 0;       // != 0: its coalesced launch failed (the wait reports rc and err)
  std::string err;
};

struct Dev;

// PublicKey.aggregate as the batch-affine pairwise tree (lsg_k_pk.hip k_agg_*, lsg_launch.h
// AggTreeArgs): L levels, T items per lane pair, n_c0 level-0 lane pairs, N0 level-0 points;
// plan arena offsets of the per-block set map, the per-set (o0, len, pk0) and k_agg_final's
// per-set sources
constexpr int64_t LSG_ITEMS_PER_BLOCK_HOST = 128;  // lane pairs per block (lsg_kcommon.hpp)
struct AggPlan {
  bool tree = false;
  int L = 0, T = 1;
  int64_t n_c0 = 0, N0 = 0;
  size_t blk_off = 0, o0_off = 0, len_off = 0, pk0_off = 0, src_off = 0;
};
constexpr size_t AGG_TREE_MIN_KEYS = 32768;  // smaller packages: the serial fold + butterfly

// (Staged, lsg_stage.hpp: what stage_sets leaves on the host -- n_sets, n_pks, pk_stride, rnd, the
// distinct messages and message-cache words, the bits and multi sets, the package's shape)
struct Slot : Staged {
  Dev* d = nullptr;
  int index = 0;
  hipStream_t st[2] = {nullptr, nullptr};  // [0] main, [1] side
  bool own_streams = true;
  // the slot's high-priority stream pair (created on first use): a package carrying an
  // LSG_JOB_PRIORITY job runs on it, so its kernels are dispatched ahead of the packages in
  // flight (verifyOnMainThread's latency under load)
  hipStream_t st_norm[2] = {nullptr, nullptr}, st_prio[2] = {nullptr, nullptr};
  int cur = 0;
  hipEvent_t ev_xp = nullptr;  // the exported partial's copy is complete (lsg_jobs_partial*)
  hipEvent_t ev_in = nullptr, ev_sig = nullptr, ev_grp = nullptr, ev_part = nullptr, ev_done = nullptr,
             ev_node = nullptr;
  // inputs (device copies of the pinned staging arena)
  DevBuf d_sig, d_siglen, d_msg, d_msgoff, d_msglen, d_pk, d_pklen, d_rnd, d_mode, d_dst;
  HostBuf h_arena;
  MsgTable mtab;  // the distinct-message table's storage, reused from package to package
  // the message cache (lsg_msg_cache_set).  mc_ok: this package may use it (set by
  // the submitter); Staged::mc_on: it was staged through it
  bool mc_ok = false;
  DevBuf d_Hx, d_hinfx;  // the misses' points when some message hit
  SegPlan msum;                  // msg_agg: per message, the masked scaled keys of the package group
  DevBuf d_mmask, d_PmP, d_Pm, d_pinfm, d_errm;
  // sets given as committee id + participation bits (LSG_PK_BITS): their
  // fields staged into the bit arena (h_cbits -> d_cbits, allocated by the first such package),
  // aggregated by k_pk_agg_bits (bplan) instead of run_pk_seg
  BitsPlan bplan;
  HostBuf h_cbits;
  DevBuf d_cbits;
  // sets given as a committee list + one bitfield (LSG_PK_BITS_MULTI): their parts' fields in the
  // same bit arena, aggregated by k_pk_agg_bits_multi (mplan) after k_pk_agg_bits
  MultiPlan mplan;
  // KeyValidate of the byte keys of LSG_JOB_VALIDATE_KEYS jobs: n_kv list items (staged key,
  // its set) in the plan arena at kv_off, kv_off + n_kv; shape.kv_set[i] != 0: set i's keys are
  // on the list (empty when the package has no such job: nothing staged, nothing launched)
  size_t n_kv = 0, kv_off = 0;
  // per-set state
  DevBuf d_ub, d_sigaff, d_siginf, d_seterr, d_pkp, d_pkerr, d_agg, d_P, d_pinf, d_H, d_hinf, d_rs, d_rs2, d_fall,
      d_fall2;
  DevBuf d_Pp, d_zP, d_zPi, d_U, d_nrm, d_nrmi, d_Hp, d_zN, d_zNi, d_mid, d_Hm, d_hinfm;
  // the stage state and the powers' operands / results of the one-element-per-lane square roots
  // (lsg_launch.h PowLanes): the signature decode's and the SSWU map's (2 items per set)
  DevBuf d_pwsig, d_pwmap;
  DevBuf binv_lv[2], binv_iv[2];
  DevBuf d_lines;
  bool rs2_ready = false;
  std::vector<uint8_t> rs2_scaled;  // per set: [r_i] sig_i is in d_rs2 (fallback phases share it)
  std::vector<uint8_t> rs_raw;      // per set: it was in a phase-A MSM group (LSG_MSM_FOLD=0: d_rs holds its unscaled point)
  // groups
  DevBuf d_S, d_F, d_verdict, d_Sb, d_fgb, d_Fb, d_bkt, d_bits, d_aux, d_gath, d_nodeF, d_nodeV;
  DevBuf seg_tmp[3][2];  // reduction scratch per use: [0] pubkeys, [1] signature sums, [2] Fp12 products
  // plan arena
  std::vector<int32_t> plan;
  HostBuf h_plan;
  DevBuf d_plan;
  PhasePlan phA;   // phase A: the package group + non-batchable jobs
  SegPlan pkagg;   // pubkey aggregation of multi-key sets (small packages)
  AggPlan agg;     // ... and as the batch-affine tree (large packages)
  DevBuf d_agga, d_aggi, d_aggpre, d_aggtot, d_aggflag;
  SegPlan phA_node;  // device 0 of a multi-device ticket: product of the gathered partials
  HostBuf h_mode;  // per-set sig_prep modes of a phase
  // pinned result mirrors
  HostBuf h_err, h_pinf, h_pkerr, h_verdict, h_blob, h_nodeV;
  std::vector<Timer> timers;
  size_t ntimers = 0;
  // ticket state
  int kind = SLOT_FREE;
  uint64_t serial = 0;
  // (Staged::shape: this device's share of the package -- jobs in staging order, sub-package
  // bounds of a coalesced launch, per-set key counts); its phase-A groups and the switches read for it
  GroupPlan gp;
  Switches sw;
  int K = 4;  // Miller pairs per item for this package
  std::vector<lsg_job_result> results;
  lsg_stats stats;
  bool has_node = false;  // this slot computed the node check (device 0 of a multi-device ticket)
  size_t n_jobs = 0;      // device 0: the ticket's job count
  // (gp.lone_unscaled: the package group is one set verified unscaled, r_i = 0, a plain verify:
  // its partial is raised to a fresh 64-bit randomizer before it leaves the slot, lsg_jobs_partial*)
  uint64_t seed = 0;  // the package's randomizer seed (0: OS CSPRNG)
  DevBuf d_xport;
  HostBuf h_xport;
  // multi-device ticket: the package group's final exponentiation was not launched -- the
  // node check over every device's partial decides, and this one runs only if that fails
  bool big_fe_pending = false;
  // coalesced launch (lsg_set_coalesce): shape.n_sub caller packages in one slot, each with
  // its own counters; the slot is freed when every sub-package's ticket has been waited on.
  std::vector<uint64_t> sub_serial;
  std::vector<lsg_stats> sub_stats;
  std::vector<int32_t> sub_pkfail;
  std::vector<uint8_t> sub_done;
  bool resolved = false, resolving = false;
  int resolve_rc = LSG_OK;
  // per-group sums of the verified signatures (lsg_submit_jobs_grouped):
  // grp_n groups (0: a plain package), set_grp[i] = staged set i's group.  The plan (gather
  // list + chunks) has an arena of its own -- the fallback phases rewrite `plan` -- and every
  // buffer here is allocated by the first grouped package (or lsg_reserve after it).
  size_t grp_n = 0;
  std::vector<uint32_t> set_grp;
  std::vector<int32_t> gplan;
  SigGroupPlan sgp;
  HostBuf h_gplan, h_gagg;
  DevBuf d_gplan, d_gsum, d_gagg, d_gtmp[2];
};

struct Dev {
  lsg_ctx* c = nullptr;
  int device = 0;
  int ord = 0;  // position in the context's device list
  hipStream_t s_util = nullptr;
  hipStream_t s_fe[LSG_FE_STREAMS] = {};
  // the node protocol's streams at the greatest priority, created on first use (idle
  // high-priority streams cost the packages hardware-queue concurrency: firehose 2.87M ->
  // ~2.4M sets/s with nine of them created up front): partial exports, node final exps
  hipStream_t s_xp = nullptr, s_nfe = nullptr;
  hipStream_t s_pp[2] = {nullptr, nullptr};  // priority packages (slot_streams), on first use
  Slot slots[LSG_SLOTS];
  Slot finals[LSG_FINALS];
  Slot util;
  // validator pubkey table (lsg_pubkey_table_set): projective lane-form keys + validity bytes
  DevBuf d_pktab, d_pktab_ok;
  size_t pktab_n = 0, pktab_cap = 0;
  // committees (lsg_committees_set): the index rows of every registered committee back to back
  // (cm_idx), per id its first row word (cm_off) and its projective sum (cm_sum, lane form);
  // lengths and the set flags are the context's (cm_len, cm_ok: the same on every device)
  DevBuf d_cm_idx, d_cm_off, d_cm_sum;
  // lsg_verify_deposits: the call's DepositData and their signing roots (the packages' messages)
  DevBuf d_dep_in, d_dep_roots;
  // the message cache (lsg_msg_cache_set): the policy, the arena of affine H(m) rows in the lane
  // layout and one infinity flag per row
  MsgCache mc;
  DevBuf d_mc_rows, d_mc_inf;
  // kernel times of the last package / call completed on this device (lsg_last_kernel_times),
  // read from the slot's timing events when it completed, before the slot can be reused
  std::vector<std::pair<const char*, float>> last_times;
};

}  // namespace

struct lsg_ctx {
  std::mutex mu;
  std::condition_variable cv;  // waiters of a coalesced slot being resolved by another thread
  std::string err;
  // Packages are staged with `mu` released (submit_pkg): `tab_mu` keeps the validator pubkey
  // table they read from changing meanwhile (shared while staging, exclusive in
  // lsg_pubkey_table_set, always taken before `mu`), `xmu` orders the RCCL exchanges of
  // packages staged at the same time, `staging` counts the submissions in flight.
  std::shared_mutex tab_mu;
  // committees (lsg_committees_set; read while staging under tab_mu shared, written under it
  // exclusively): per id its length, set flag and first word in cm_rows, the host copy of the
  // devices' index rows (replaced and cleared committees leave dead words behind: cm_dead;
  // compacted when they outweigh the live ones)
  std::vector<uint32_t> cm_len, cm_off, cm_rows;
  std::vector<uint8_t> cm_ok;
  size_t cm_dead = 0;
  std::mutex xmu;
  std::mutex dep_mu;  // one lsg_verify_deposits at a time (they share d_dep_*), taken before `mu`
  int staging = 0;
  // coalescing (lsg_set_coalesce): packages of <= co_max_sets sets wait in `pending` while
  // co_inflight launches are on the device, then go out as one launch
  uint32_t co_max_sets = 0;
  int co_inflight = 2;
  size_t co_max_pending = 16384;
  std::vector<PendingPkg> pending;
  size_t pending_sets = 0;
  std::unordered_map<uint64_t, MergeTicket> merged;
  bool grouped_seen = false;  // a grouped package was submitted: lsg_reserve sizes the group buffers too
  int n_dev = 0;
  Dev* dev[LSG_MAX_DEVICES] = {};
  bool rccl = false;  // several distinct devices: the partials are all-gathered over RCCL
  ncclComm_t comm[LSG_MAX_DEVICES] = {};
  uint64_t next_serial = 1;
};

namespace {

// A thread staging a package without the context lock reports its errors here; the
// submitter copies them into c->err once it holds the lock again (submit_pkg).
thread_local std::string* t_err_sink = nullptr;
void set_err(lsg_ctx* c, std::string m) {
  if (t_err_sink)
    *t_err_sink = std::move(m);
  else
    c->err = std::move(m);
}

int fail_c(lsg_ctx* c, const char* what, hipError_t e) {
  set_err(c, std::string(what) + ": " + hipGetErrorString(e));
  return LSG_ERR_DEVICE;
}
int fail(Slot* s, const char* what, hipError_t e) { return fail_c(s->d->c, what, e); }

#define LSG_HIP(s, call)                               \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return fail((s), #call, _e); \
  } while (0)
#define LSG_HIPC(c, call)                                \
  do {                                                   \
    hipError_t _e = (call);                              \
    if (_e != hipSuccess) return fail_c((c), #call, _e); \
  } while (0)
#define LSG_RC(call)         \
  do {                       \
    int _rc = (call);        \
    if (_rc) return _rc;     \
  } while (0)

int ensure(Slot* s, DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 64;
  if (b.cap >= bytes) return LSG_OK;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t cap = std::max(bytes + bytes / 4, (size_t)4096);
  hipError_t e = hipMalloc(&b.p, cap);
  if (e != hipSuccess) return fail(s, "hipMalloc", e);
  g_allocs++;
  trace_alloc("device", cap);
  b.cap = cap;
  return LSG_OK;
}

int ensure_host(Slot* s, HostBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 64;
  if (b.cap >= bytes) return LSG_OK;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t cap = std::max(bytes + bytes / 4, (size_t)4096);
  hipError_t e = hipHostMalloc(&b.p, cap, hipHostMallocDefault);
  if (e != hipSuccess) return fail(s, "hipHostMalloc", e);
  g_allocs++;
  trace_alloc("pinned", cap);
  b.cap = cap;
  return LSG_OK;
}

void free_dev(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}
void free_host(HostBuf& b) {
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

template <class T>
T* P_(const DevBuf& b) {
  return (T*)b.p;
}
template <class T>
T* H_(const HostBuf& b) {
  return (T*)b.p;
}

inline hipStream_t S_(Slot* s) { return s->st[s->cur]; }

void timer_reset(Slot* s) {
  s->ntimers = 0;
  s->cur = 0;
}
void timer_begin(Slot* s, const char* name) {
  if (s->ntimers >= s->timers.size()) {
    Timer t;
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    s->timers.push_back(t);
  }
  Timer& t = s->timers[s->ntimers];
  t.name = name;
  (void)hipEventRecord(t.a, S_(s));
}
void timer_end(Slot* s) {
  (void)hipEventRecord(s->timers[s->ntimers].b, S_(s));
  s->ntimers++;
}

// a launch through lsg_launch.h on the slot's current stream, timed with HIP events
#define KL(s, name, call)                                 \
  do {                                                    \
    timer_begin((s), name);                               \
    hipError_t _le = (call);                              \
    timer_end((s));                                       \
    if (_le != hipSuccess) return fail((s), name, _le);   \
  } while (0)

// device pointer of arena word `off`
inline const int32_t* PL(Slot* s, size_t off) { return P_<int32_t>(s->d_plan) + off; }

// snapshot a completed slot's kernel times for lsg_last_kernel_times (-1: not measured)
void keep_times(Slot* s) {
  auto& v = s->d->last_times;
  v.clear();
  for (size_t i = 0; i < s->ntimers; i++) {
    float t = 0;
    if (hipEventElapsedTime(&t, s->timers[i].a, s->timers[i].b) != hipSuccess) t = -1;
    v.push_back({s->timers[i].name, t});
  }
}

// a greatest-priority stream of the device, created on first use
int prio_stream(lsg_ctx* c, Dev* d, hipStream_t* st) {
  if (!*st) {
    int least = 0, greatest = 0;
    LSG_HIPC(c, hipSetDevice(d->device));
    LSG_HIPC(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    LSG_HIPC(c, hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest));
  }
  return LSG_OK;
}

// Host wait for a completion event without holding a core: hipEventSynchronize spins on this
// stack (with hipEventBlockingSync too: the gossip bench's 64 waiter threads kept 16 cores
// busy, tools/thread_cpu.py), so poll -- back to back for the first 20 us, then with 30 us
// sleeps; the added latency is well under 0.1 ms per wait.
hipError_t event_wait(hipEvent_t e) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t r = hipEventQuery(e);
    if (r != hipErrorNotReady) return r;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(20))
      std::this_thread::sleep_for(std::chrono::microseconds(30));
  }
}

// LSG_BLOCKING_WAITS=1: waiters sleep on the completion events (hipEventBlockingSync)
bool blocking_waits() {
  const char* e = getenv("LSG_BLOCKING_WAITS");
  return e && atoi(e) != 0;
}

int slot_create(Dev* d, Slot* s, int index, hipStream_t shared) {
  s->d = d;
  s->index = index;
  if (shared) {
    s->st[0] = s->st[1] = shared;
    s->own_streams = false;
  } else {
    for (int k = 0; k < 2; k++) LSG_HIP(s, hipStreamCreateWithFlags(&s->st_norm[k], hipStreamNonBlocking));
    s->st[0] = s->st_norm[0];
    s->st[1] = s->st_norm[1];
  }
  hipEvent_t* evs[] = {&s->ev_in, &s->ev_sig, &s->ev_grp, &s->ev_part, &s->ev_done, &s->ev_node, &s->ev_xp};
  for (hipEvent_t* e : evs) LSG_HIP(s, hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (blocking_waits()) {  // the events a waiter blocks on: sleep instead of spinning
    for (hipEvent_t* e : {&s->ev_part, &s->ev_done}) {
      LSG_HIP(s, hipEventDestroy(*e));
      LSG_HIP(s, hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventBlockingSync));
    }
  }
  LSG_RC(ensure(s, s->d_dst, 256));
  LSG_HIP(s, hipMemcpy(s->d_dst.p, DST_POP, DST_POP_LEN, hipMemcpyHostToDevice));
  return LSG_OK;
}

void slot_destroy(Slot* s) {
  if (!s->d) return;
  for (int k = 0; k < 2; k++)
    if (s->st[k]) (void)hipStreamSynchronize(s->st[k]);
  DevBuf* bufs[] = {&s->d_sig,  &s->d_siglen, &s->d_msg,  &s->d_msgoff, &s->d_msglen, &s->d_pk,    &s->d_pklen,
                    &s->d_rnd,  &s->d_mode,   &s->d_dst,  &s->d_ub,     &s->d_sigaff, &s->d_siginf, &s->d_seterr,
                    &s->d_pkp,  &s->d_pkerr,  &s->d_agg,  &s->d_P,      &s->d_pinf,   &s->d_H,     &s->d_hinf,
                    &s->d_rs,   &s->d_rs2,    &s->d_fall, &s->d_fall2,  &s->d_Pp,     &s->d_zP,    &s->d_zPi,
                    &s->d_U,    &s->d_nrm,    &s->d_nrmi, &s->d_Hp,     &s->d_zN,     &s->d_zNi,   &s->binv_lv[0],
                    &s->binv_lv[1], &s->binv_iv[0], &s->binv_iv[1], &s->d_lines, &s->d_S, &s->d_F, &s->d_verdict,
                    &s->d_Sb,   &s->d_fgb,    &s->d_Fb,   &s->d_bkt,    &s->d_bits,   &s->d_aux,   &s->d_gath,
                    &s->d_nodeF, &s->d_nodeV, &s->d_plan, &s->d_mid, &s->d_Hm, &s->d_hinfm,
                    &s->d_mmask, &s->d_PmP, &s->d_Pm, &s->d_pinfm, &s->d_errm, &s->d_xport,
                    &s->d_agga, &s->d_aggi, &s->d_aggpre, &s->d_aggtot, &s->d_aggflag, &s->d_cbits,
                    &s->d_gplan, &s->d_gsum, &s->d_gagg, &s->d_gtmp[0], &s->d_gtmp[1], &s->d_Hx, &s->d_hinfx,
                    &s->d_pwsig, &s->d_pwmap};
  for (DevBuf* b : bufs) free_dev(*b);
  for (auto& u : s->seg_tmp)
    for (DevBuf& b : u) free_dev(b);
  HostBuf* hb[] = {&s->h_arena, &s->h_err, &s->h_pinf, &s->h_pkerr, &s->h_verdict, &s->h_blob, &s->h_plan, &s->h_nodeV,
                   &s->h_xport, &s->h_cbits, &s->h_gplan, &s->h_gagg};
  for (HostBuf* b : hb) free_host(*b);
  for (Timer& t : s->timers) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  s->timers.clear();
  hipEvent_t evs[] = {s->ev_in, s->ev_sig, s->ev_grp, s->ev_part, s->ev_done, s->ev_node, s->ev_xp};
  for (hipEvent_t e : evs)
    if (e) (void)hipEventDestroy(e);
  if (s->own_streams) {
    for (int k = 0; k < 2; k++) {
      if (s->st_prio[k]) (void)hipStreamSynchronize(s->st_prio[k]);
      if (s->st_norm[k]) (void)hipStreamSynchronize(s->st_norm[k]);
    }
    for (int k = 0; k < 2; k++) {
      if (s->st_norm[k]) (void)hipStreamDestroy(s->st_norm[k]);
      // (st_prio: the device's shared pair, destroyed with the device)
      s->st_norm[k] = s->st_prio[k] = s->st[k] = nullptr;
    }
  }
  s->d = nullptr;
}

// select the slot's stream pair for its next package (the slot is free: nothing of an
// earlier package is in flight on either pair)
int slot_streams(Slot* s, bool prio) {
  if (!s->own_streams) return LSG_OK;
  // priority packages share one pair of greatest-priority streams per device, created on
  // first use: a pair per slot would leave idle high-priority streams behind that take
  // hardware-queue concurrency from every later package
  if (prio && !s->st_prio[0]) {
    Dev* d = s->d;
    for (int k = 0; k < 2; k++) LSG_RC(prio_stream(d->c, d, &d->s_pp[k]));
    s->st_prio[0] = d->s_pp[0];
    s->st_prio[1] = d->s_pp[1];
  }
  hipStream_t* p = prio ? s->st_prio : s->st_norm;
  s->st[0] = p[0];
  s->st[1] = p[1];
  return LSG_OK;
}

// the pipeline slot `s` of device `d`, created on first use
int slot_ready(Dev* d, Slot* s, int index) {
  if (s->d) return LSG_OK;
  const int rc = slot_create(d, s, index, nullptr);
  if (rc) slot_destroy(s);
  return rc;
}

// ---- sizes
// Miller pairs per item (one shared f and its squarings): K = 4 does the least work per set,
// but one item is one lane pair, so a small package has few items and its accumulation wave
// runs alone for ~14 ms; smaller K trades work for latency there.  Env LSG_MILLER_K forces K.
// The fused Miller kernel (k_miller_fused: lines in LDS, four waves per item of four pairs) is
// the default; LSG_MILLER_FUSED=0 selects the split pair k_miller_lines / k_miller_accum<K>.
bool miller_fused() { return lsg_ab_long("LSG_MILLER_FUSED", 1) != 0; }
// k_miller_fused runs with one Fp2 component per lane (lsg_fp2_lanes.hpp); LSG_MF_LANES=0 (A/B
// build): its pair-form twin k_miller_fused_pair
static bool mf_lanes_on() { return lsg_ab_long("LSG_MF_LANES", 1) != 0; }

size_t slp_items_max();
int miller_k_for(size_t n_sets) {
  if (miller_fused()) return n_sets <= slp_items_max() ? 1 : 4;  // fused: four waves' lane pairs per item
  const long v = lsg_ab_long("LSG_MILLER_K", 0);
  if (v == 1 || v == 2 || v == 4) return (int)v;
  return n_sets >= 8192 ? 4 : (n_sets >= 1024 ? 2 : 1);
}

// PublicKey.aggregate of large packages as the batch-affine tree: A/B build only
// (LSG_AGG_TREE=1).  Measured slower than the fused gather + mixed-addition fold
// (k_pk_agg_seg) on config C: 2.7 ms against 1.44 ms for a 3.7M-key block package alone,
// 0.90M against 0.98M sets/s loaded -- the per-level inversion, heap and
// point round trips cost more than the four products per key the affine additions save.
bool agg_tree_on() { return lsg_ab_long("LSG_AGG_TREE", 0) != 0; }

// The switches of lsg_plan.hpp's plans and verdict rules (the A/B build reads the environment
// here, once per package: pkg_part1; the shipped library's values are constants).
// LSG_MSM_MIN_GROUP, the minimum RLC group size for the bucket MSM: by operation count the MSM
// wins from ~4 sets (2-bit windows: ~24 bucket additions plus 4 of the group's 64 bit sums, ~1k
// Fp products, against ~2.25k for a 64-bit scalar multiplication; the group's Horner program
// ~4k more), but the per-set [r_i] sig_i kernel runs near 0.3 of the mad peak and the bucket
// and bit-sum reductions far below it, plus a Horner program per group: on config C (64 groups
// of 128 sets) 1.05-1.08M sets/s without the MSM against 1.01M with it
// (profiles/r04_msm_ab.txt).  The MSM stays for groups of 256 and more (8-bit windows: the
// firehose's package group, the fallback phases' halves).
// LSG_PACKAGE_GROUP=0: phase A as the reference batches it, one RLC group per 16-job chunk
// instead of one package group (A/B and the equivalence test of the two modes).
// LSG_SUB_GROUPS=0: a coalesced launch as round 3's one group per 16-job chunk instead of one
// package group per sub-package.
// LSG_NB_MERGE=0: one group per non-batchable job instead of ONE RLC group for all of them
// (>= 2 with sets), localised per job only when it fails.  Each job's verdict is its own
// validity either way (worker.ts:88-96: such a job is verified alone), and non-batchable jobs
// never enter the batch counters.
// LSG_B0_MIN / LSG_B0_RUN (phase B0): with at least B0_MIN chunks to check, runs of up to B0_RUN
// consecutive chunks are checked as one group first (0: off).
// LSG_MSG_AGG=0: one Miller pair per set instead of one per distinct message in the package
// group (read per package, so that a test can compare both forms in one process).
Switches read_switches() {
  Switches w;
  w.package_group = lsg_ab_long("LSG_PACKAGE_GROUP", 1) != 0;
  w.sub_groups = lsg_ab_long("LSG_SUB_GROUPS", 1) != 0;
  w.nb_merge = lsg_ab_long("LSG_NB_MERGE", 1) != 0;
  w.msg_agg = lsg_ab_long("LSG_MSG_AGG", 1) != 0;
  w.msm_min_group = (size_t)std::max(1L, lsg_ab_long("LSG_MSM_MIN_GROUP", 256));
  w.b0_min = (size_t)std::max(0L, lsg_ab_long("LSG_B0_MIN", 64));
  w.b0_run = (size_t)std::max(2L, lsg_ab_long("LSG_B0_RUN", 4));
  w.seg_fold_wide = (int)lsg_ab_long("LSG_SEG_FOLD_WIDE", SEG_FOLD_WIDE);
  w.slp_items = slp_items_max();
  w.msm_fold = lsg_ab_long("LSG_MSM_FOLD", LSG_MSM_FOLD_DEFAULT) != 0;
  w.msm_ips = (int)std::max(-1L, std::min(lsg_ab_long("LSG_MSM_IPS", LSG_MSM_IPS_DEFAULT), 5L));
  return w;
}
// plan_seg for a slot's plan arena
SegPlan slot_seg(Slot* s, int op, const std::vector<int32_t>& seg_off, const std::vector<int32_t>& seg_len, bool has_idx,
                 size_t idx_off, int32_t dst_base) {
  return plan_seg(s->plan, op, seg_off, seg_len, has_idx, idx_off, dst_base,
                  (int)lsg_ab_long("LSG_SEG_FOLD_WIDE", SEG_FOLD_WIDE));
}

void binv_sizes(size_t n, size_t* lv, size_t* iv);
size_t binv_lv_words(size_t n) {
  size_t a, b;
  binv_sizes(n, &a, &b);
  return a;
}
size_t binv_iv_words(size_t n) {
  size_t a, b;
  binv_sizes(n, &a, &b);
  return b;
}

// inputs for up to n sets / np keys / mb message bytes
int size_inputs(Slot* s, size_t n, size_t np, size_t mb) {
  const size_t nn = std::max(n, (size_t)1), pp = std::max(np, (size_t)1);
  LSG_RC(ensure_host(s, s->h_arena, stage_layout(n, np, 96, mb).bytes));  // (96: the wider key slot)
  LSG_RC(ensure(s, s->d_sig, 192 * nn));
  LSG_RC(ensure(s, s->d_siglen, 4 * nn));
  LSG_RC(ensure(s, s->d_msg, std::max(mb, (size_t)1)));
  LSG_RC(ensure(s, s->d_msgoff, 4 * nn));
  LSG_RC(ensure(s, s->d_msglen, 4 * nn));
  LSG_RC(ensure(s, s->d_pk, 96 * pp));
  LSG_RC(ensure(s, s->d_pklen, 4 * pp));
  LSG_RC(ensure(s, s->d_rnd, 8 * nn));
  LSG_RC(ensure(s, s->d_mode, nn));
  LSG_RC(ensure(s, s->d_mid, 4 * nn));
  return LSG_OK;
}

// per-set state and group buffers for n sets / np keys / ng groups (n_msm of them bucket-MSM
// groups) in any phase
// pkg: 0 utility calls; 1 phase A of a package (every per-set buffer); 2 a fallback phase
// (only its own buffers: the per-set state of phase A stays resident and is never moved)
int size_state(Slot* s, size_t n, size_t np, size_t ng, size_t n_msm, int pkg = 0) {
  const size_t nn = std::max(n, (size_t)1), pp = std::max(np, (size_t)1), gg = std::max(ng, (size_t)1);
  const size_t g_msm = std::max(n_msm, (size_t)1);
  struct {
    DevBuf* b;
    size_t bytes;
  } dev[] = {{&s->d_ub, 256 * nn},
             {&s->d_sigaff, 4 * W_G2A * nn},
             {&s->d_siginf, nn},
             {&s->d_seterr, 4 * nn},
             {&s->d_pkp, 4 * W_G1P * pp},
             {&s->d_pkerr, 4 * pp},
             {&s->d_agg, 4 * W_G1P * nn},
             {&s->d_P, 4 * W_G1A * nn},
             {&s->d_pinf, nn},
             {&s->d_H, 4 * W_G2A * nn},
             {&s->d_hinf, nn},
             {&s->d_rs, 4 * W_G2P * nn},
             {&s->d_Pp, 4 * W_G1P * nn},
             {&s->d_zP, 4 * W_FP * nn},
             {&s->d_zPi, 4 * W_FP * nn},
             {&s->d_U, 4 * W_H2CU * nn},
             {&s->d_nrm, 4 * W_FP * 2 * nn},
             {&s->d_nrmi, 4 * W_FP * 2 * nn},
             {&s->d_Hp, 4 * W_G2P * nn},
             {&s->d_zN, 4 * W_FP * nn},
             {&s->d_zNi, 4 * W_FP * nn},
             {&s->d_pwsig, 4 * (lsgk::POW_SIG_STATE + 2 * W_FP) * nn},
             {&s->d_pwmap, 4 * (lsgk::POW_MAP_STATE + 2 * W_FP) * 2 * nn},
             {&s->binv_lv[0], 4 * W_FP * binv_lv_words(2 * nn)},
             {&s->binv_iv[0], 4 * W_FP * binv_iv_words(2 * nn)},
             {&s->binv_lv[1], 4 * W_FP * binv_lv_words(nn)},
             {&s->binv_iv[1], 4 * W_FP * binv_iv_words(nn)},
             {&s->d_S, 4 * W_G2P * gg},
             {&s->d_F, 4 * W_F12 * gg},
             {&s->d_verdict, 4 * gg},
             {&s->d_Sb, (size_t)288 * (MSM_BITS * g_msm + gg)},
             {&s->d_fgb, 576 * gg},
             {&s->d_Fb, 576 * gg},
             {&s->d_bkt, 4 * W_G2P * (size_t)MSM_WINDOWS * MSM_DIGITS * g_msm},
             {&s->d_bits, 4 * W_G2P * (size_t)MSM_BITS * g_msm},
             {&s->d_gath, 576 * (LSG_MAX_DEVICES + 2)},  // partials, the identity, the node product
             {&s->d_nodeF, 4 * W_F12 * (LSG_MAX_DEVICES + 1)},
             {&s->d_nodeV, 64}};
  for (auto& x : dev) LSG_RC(ensure(s, *x.b, x.bytes));
  if (pkg == 1) {  // Miller lines (split kernels only) and items; fall also holds phase B's chunk terms
    if (!miller_fused()) LSG_RC(ensure(s, s->d_lines, 4 * (size_t)ML_STEPS * W_LINE * nn));
    // items, phase A's group terms, then the terms of a reusing phase (phase B's chunks, or
    // phase C's item-aligned job groups: at most one per item)
    LSG_RC(ensure(s, s->d_fall, 4 * W_F12 * (2 * nn + gg + 2)));
  }
  if (pkg) {  // fallback signature sums and Miller items: a phase C of single-set jobs needs
              // one item and one term slot per retried set
    LSG_RC(ensure(s, s->d_fall2, 4 * W_F12 * (nn + std::max(gg, nn))));
    LSG_RC(ensure(s, s->d_rs2, 4 * W_G2P * nn));
  }
  LSG_RC(ensure_host(s, s->h_err, 4 * nn));
  LSG_RC(ensure_host(s, s->h_pinf, nn));
  LSG_RC(ensure_host(s, s->h_pkerr, 4 * pp));
  LSG_RC(ensure_host(s, s->h_verdict, 4 * gg));
  LSG_RC(ensure_host(s, s->h_blob, 576 * gg));
  LSG_RC(ensure_host(s, s->h_nodeV, 64));
  return LSG_OK;
}

// reduction scratch for a plan
int size_seg(Slot* s, int use, const SegPlan& P) {
  if (P.tmp_items == 0) return LSG_OK;
  const size_t W = P.op == 0 ? W_G1P : (P.op == 1 ? W_G2P : W_F12);
  LSG_RC(ensure(s, s->seg_tmp[use][0], 4 * W * P.tmp_items));
  return ensure(s, s->seg_tmp[use][1], 4 * W * P.tmp_items);
}

// upload the plan arena (one copy on the main stream, before ev_in)
int upload_plan(Slot* s) {
  const size_t bytes = 4 * std::max(s->plan.size(), (size_t)1);
  LSG_RC(ensure_host(s, s->h_plan, bytes));
  LSG_RC(ensure(s, s->d_plan, bytes));
  if (!s->plan.empty()) {
    memcpy(s->h_plan.p, s->plan.data(), 4 * s->plan.size());
    LSG_HIP(s, hipMemcpyAsync(s->d_plan.p, s->h_plan.p, 4 * s->plan.size(), hipMemcpyHostToDevice, s->st[0]));
  }
  return LSG_OK;
}

// run a planned reduction on the current stream; use selects the scratch pair
int run_seg(Slot* s, int use, const char* name, const SegPlan& P, const uint32_t* src, uint32_t* dst) {
  LSG_RC(size_seg(s, use, P));
  uint32_t* tmp[3] = {nullptr, P_<uint32_t>(s->seg_tmp[use][0]), P_<uint32_t>(s->seg_tmp[use][1])};
  const int32_t* idx = P.has_idx ? PL(s, P.idx_off) : nullptr;
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    const uint32_t* in = q.src == 0 ? src : tmp[q.src];
    KL(s, name, lsgk::seg_reduce(S_(s), P.op, q.n_chunks, q.ips_log2, PL(s, q.chunk_off), k == 0 ? idx : nullptr, in, dst,
                                 tmp[q.tmp_out]));
  }
  return LSG_OK;
}

// PublicKey.aggregate of the slot's multi-key sets by the segmented reduction, its first pass
// fetching the staged keys itself (lsg_k_pk.hip k_pk_agg_seg; P = plan_pk_agg)
int run_pk_seg(Slot* s, const SegPlan& P, uint32_t* dst) {
  LSG_RC(size_seg(s, 0, P));
  Dev* d = s->d;
  uint32_t* tmp[3] = {nullptr, P_<uint32_t>(s->seg_tmp[0][0]), P_<uint32_t>(s->seg_tmp[0][1])};
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    if (k == 0)
      KL(s, "g1_aggregate", lsgk::pk_agg_seg(S_(s), q.n_chunks, q.ips_log2, PL(s, q.chunk_off), P_<uint8_t>(s->d_pk),
                                             s->pk_stride, P_<uint32_t>(s->d_pklen), P_<int32_t>(s->d_pkerr),
                                             P_<uint32_t>(d->d_pktab), P_<uint8_t>(d->d_pktab_ok), (uint32_t)d->pktab_n,
                                             dst, tmp[q.tmp_out]));
    else
      KL(s, "g1_aggregate", lsgk::seg_reduce(S_(s), 0, q.n_chunks, q.ips_log2, PL(s, q.chunk_off), nullptr,
                                             tmp[q.src], dst, tmp[q.tmp_out]));
  }
  return LSG_OK;
}

// ---- per-group sums of the verified signatures (lsg_submit_jobs_grouped)
// buffers for n sets in ng groups: the plan arena (the gather list, at most n words plus n / 8
// of padding, and three words per chunk: one per group or per SEG_FOLD members in the first
// pass, fewer in the second), the chunk sums of groups longer than a chunk, the projective sums and the output
int size_groups(Slot* s, size_t n, size_t ng) {
  const size_t words = 2 * n + 3 * ng + 64, tmp_items = n / 8 + 64;
  LSG_RC(ensure_host(s, s->h_gplan, 4 * words));
  LSG_RC(ensure(s, s->d_gplan, 4 * words));
  for (DevBuf& b : s->d_gtmp) LSG_RC(ensure(s, b, 4 * W_G2P * tmp_items));
  LSG_RC(ensure(s, s->d_gsum, 4 * W_G2P * std::max(ng, (size_t)1)));
  LSG_RC(ensure(s, s->d_gagg, 96 * std::max(ng, (size_t)1)));
  LSG_RC(ensure_host(s, s->h_gagg, 96 * std::max(ng, (size_t)1)));
  s->gplan.reserve(words);
  return LSG_OK;
}

// Plan, upload and launch the group sums of the slot's package on the current stream: per
// group the sum of its sets' resident affine signatures (mask: only sets with mask[i] != 0;
// null: every grouped set), compressed into h_gagg.  No host synchronisation.
int run_sig_groups(Slot* s, const uint8_t* mask) {
  const size_t ng = s->grp_n;
  s->gplan.clear();
  s->sgp = plan_sig_groups(s->gplan, s->set_grp.data(), s->n_sets, ng, mask,
                           (int)lsg_ab_long("LSG_SEG_FOLD_WIDE", SEG_FOLD_WIDE));
  const SegPlan& P = s->sgp.seg;
  const size_t bytes = 4 * std::max(s->gplan.size(), (size_t)1);
  LSG_RC(ensure_host(s, s->h_gplan, bytes));
  LSG_RC(ensure(s, s->d_gplan, bytes));
  for (DevBuf& b : s->d_gtmp) LSG_RC(ensure(s, b, 4 * W_G2P * std::max(P.tmp_items, (size_t)1)));
  LSG_RC(ensure(s, s->d_gsum, 4 * W_G2P * ng));
  LSG_RC(ensure(s, s->d_gagg, 96 * ng));
  LSG_RC(ensure_host(s, s->h_gagg, 96 * ng));
  memcpy(s->h_gplan.p, s->gplan.data(), 4 * s->gplan.size());
  LSG_HIP(s, hipMemcpyAsync(s->d_gplan.p, s->h_gplan.p, 4 * s->gplan.size(), hipMemcpyHostToDevice, S_(s)));
  const int32_t* A = P_<int32_t>(s->d_gplan);
  uint32_t* tmp[3] = {nullptr, P_<uint32_t>(s->d_gtmp[0]), P_<uint32_t>(s->d_gtmp[1])};
  uint32_t* dst = P_<uint32_t>(s->d_gsum);
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    if (k == 0)
      KL(s, "k_sig_agg_seg", lsgk::sig_agg_seg(S_(s), q.n_chunks, q.ips_log2, A + q.chunk_off, A + s->sgp.gather_off,
                                               P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                               P_<int32_t>(s->d_seterr), dst, tmp[q.tmp_out]));
    else
      KL(s, "sig_agg_reduce", lsgk::seg_reduce(S_(s), 1, q.n_chunks, q.ips_log2, A + q.chunk_off, nullptr, tmp[q.src], dst,
                                               tmp[q.tmp_out]));
  }
  KL(s, "k_g2p_compress", lsgk::g2p_compress(S_(s), (int)ng, dst, P_<uint8_t>(s->d_gagg)));
  LSG_HIP(s, hipMemcpyAsync(s->h_gagg.p, s->d_gagg.p, 96 * ng, hipMemcpyDeviceToHost, S_(s)));
  return LSG_OK;
}

// batched inversions in one launch per call (k_binv_block); LSG_BINV_BLOCK=0 (A/B build): the
// multi-level fold / root / unfold launches
static bool binv_block_on() { return lsg_ab_long("LSG_BINV_BLOCK", 1) != 0; }
// the G2 [x] chains of k_sig_subgroup and k_h2c_clear with one Fp2 component per lane
// (lsg_fp2_lanes.hpp); LSG_FP2_LANES=0 (A/B build): the kernels' pair-form twins
static bool fp2_lanes_on() { return lsg_ab_long("LSG_FP2_LANES", 1) != 0; }
// The square-root powers of sig_decode and h2c_map with one element per lane (k_fp_pow_lanes)
// from LSG_POW_LANES_MIN power operands per launch on (one per signature, two per message); below
// it the single pair-form kernels, whose latency a lone set or a small package keeps.  The
// default is a wave of the power kernel for every SIMD of the device (65,536 elements): with
// fewer, a launch alone on the device lasts as long as one wave, and a lane-form power is 1.65
// times the pair form's instructions (profiles/r17_powlanes_threshold.txt).  b: the slot's
// scratch for `items` items of `state` words.
lsgk::PowLanes pow_lanes(const DevBuf& b, size_t items, size_t state) {
  lsgk::PowLanes pw;
  if (lsg_ab_long("LSG_POW_LANES", LSG_POW_LANES_DEFAULT) == 0 || b.cap < 4 * (state + 2 * W_FP) * items) return pw;
  pw.min_items = (int)std::max(1L, std::min(lsg_ab_long("LSG_POW_LANES_MIN", LSG_POW_LANES_MIN_DEFAULT), 0x7fffffffL));
  pw.state = P_<uint32_t>(b);
  pw.pa = pw.state + state * items;
  pw.pb = pw.pa + W_FP * items;
  return pw;
}
// a zero-length entry of the kernel times when the launch ran the lane-form powers: the stage
// labels k_sig_decode and k_h2c_map cover their whole wrapper on either path
#define KL_POW(s, pw, items)                                          \
  do {                                                                \
    if ((pw).on((int)(items))) KL(s, "k_fp_pow_lanes", hipSuccess);   \
  } while (0)

// G2 membership of the slot's n decoded signatures (d_sigaff, d_siginf) into d_seterr
int launch_sig_subgroup(Slot* s, int n) {
  if (fp2_lanes_on())
    KL(s, "k_sig_subgroup", lsgk::sig_subgroup(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                               P_<int32_t>(s->d_seterr)));
  else
    KL(s, "k_sig_subgroup_pair", lsgk::sig_subgroup(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                                    P_<int32_t>(s->d_seterr), true));
  return LSG_OK;
}

// Words (per Fp of W_FP) of the two scratch arrays a batched inversion of n values needs:
// lv = every level's prefix products plus levels >= 1's values, iv = levels >= 1's inverses
void binv_sizes(size_t n, size_t* lv, size_t* iv) {
  size_t a = 0, b = 0;
  for (size_t m = n; m > 1;) {
    const size_t up = (m + LSG_BINV_T - 1) / LSG_BINV_T;
    a += m + up;
    b += up;
    m = up;
  }
  *lv = std::max(a, (size_t)1);
  *iv = std::max(b, (size_t)1);
}

// out[i] = 1 / v[i] (0 for v[i] = 0) for n lane-form Fp values on the current stream
// (Montgomery's trick in chunks of LSG_BINV_T per lane pair: lsg_k_reduce.hip)
int batch_inv(Slot* s, int ws, const char* name, const uint32_t* v, size_t n, uint32_t* out) {
  if (n == 0) return LSG_OK;
  size_t lvw, ivw;
  binv_sizes(n, &lvw, &ivw);
  LSG_RC(ensure(s, s->binv_lv[ws], 4 * W_FP * lvw));
  LSG_RC(ensure(s, s->binv_iv[ws], 4 * W_FP * ivw));
  uint32_t* lv = P_<uint32_t>(s->binv_lv[ws]);
  uint32_t* iv = P_<uint32_t>(s->binv_iv[ws]);
  if (binv_block_on()) {  // one launch: a divstep root per block of 128 x T values
    // ~64 blocks: each holds its CU slot through one ~30 us divstep root (and the heap's
    // barriers), so fewer, longer blocks cost the loaded GPU less than one block per 128 values
    // (7 % of summed kernel time with T = 1, profiles/r05_rocprof_stats_a.csv)
    const int T = (int)std::min<size_t>(64, std::max<size_t>(1, (n + 128 * 64 - 1) / (128 * 64)));
    KL(s, name, lsgk::binv_block(S_(s), (int)n, T, 1, v, lv, out));
    return LSG_OK;
  }
  // level l: values val[l] (val[0] = v), prefix products pre[l], inverses inv[l] (inv[0] = out)
  std::vector<size_t> cnt{n};
  std::vector<uint32_t*> val{(uint32_t*)v}, pre, inv{out};
  size_t lo = 0, io = 0;
  while (cnt.back() > 1) {
    const size_t m = cnt.back(), up = (m + LSG_BINV_T - 1) / LSG_BINV_T;
    pre.push_back(lv + W_FP * lo);
    lo += m;
    val.push_back(lv + W_FP * lo);
    lo += up;
    inv.push_back(iv + W_FP * io);
    io += up;
    cnt.push_back(up);
  }
  const size_t L = cnt.size() - 1;
  if (L == 0) {  // one value: invert it directly (0 stays 0)
    KL(s, name, lsgk::binv_root(S_(s), v, out));
    return LSG_OK;
  }
  for (size_t l = 0; l < L; l++)
    KL(s, name, lsgk::binv_fold(S_(s), (int)cnt[l], l == 0 ? 1 : 0, val[l], pre[l], val[l + 1]));
  KL(s, name, lsgk::binv_root(S_(s), val[L], inv[L]));
  for (size_t l = L; l-- > 0;)
    KL(s, name, lsgk::binv_unfold(S_(s), (int)cnt[l], l == 0 ? 1 : 0, val[l], pre[l], inv[l + 1], inv[l]));
  return LSG_OK;
}

// Packages of up to LSG_SLP_ITEMS sets (default 2048; 0: never) run one-set Miller items as
// straight-line programs (lsg_slp.hip, one workgroup per set, ~0.8 ms) instead of the fused
// kernel, whose latency is one full loop per lane whatever the package size (~5.4 ms).

size_t slp_items_max() {
  const long v = lsg_ab_long("LSG_SLP_ITEMS", 2048);
  return v > 0 ? (size_t)v : 0;
}

// hash_to_G2 of the slot's n expanded messages (d_ub) into H / hinf on the current stream
int launch_hash(Slot* s, int n, uint32_t* H, uint8_t* hinf) {
  KL(s, "k_h2c_prep", lsgk::h2c_prep(S_(s), n, P_<uint8_t>(s->d_ub), P_<uint32_t>(s->d_U), P_<uint32_t>(s->d_nrm)));
  LSG_RC(batch_inv(s, 0, "binv_sswu", P_<uint32_t>(s->d_nrm), 2 * (size_t)n, P_<uint32_t>(s->d_nrmi)));
  const lsgk::PowLanes pw = pow_lanes(s->d_pwmap, 2 * (size_t)n, lsgk::POW_MAP_STATE);
  KL(s, "k_h2c_map", lsgk::h2c_map(S_(s), n, P_<uint32_t>(s->d_U), P_<uint32_t>(s->d_nrmi), P_<uint32_t>(s->d_Hp), pw));
  KL_POW(s, pw, 2 * (size_t)n);
  if ((size_t)n <= slp_items_max()) {  // small packages: clearing + affine as one program per set
    KL(s, "k_slp_h2c", lsg_slp_h2c_clear(S_(s), n, P_<uint32_t>(s->d_Hp), H, hinf));
    return LSG_OK;
  }
  if (fp2_lanes_on())
    KL(s, "k_h2c_clear", lsgk::h2c_clear(S_(s), n, P_<uint32_t>(s->d_Hp), P_<uint32_t>(s->d_zN), hinf));
  else
    KL(s, "k_h2c_clear_pair", lsgk::h2c_clear(S_(s), n, P_<uint32_t>(s->d_Hp), P_<uint32_t>(s->d_zN), hinf, true));
  LSG_RC(batch_inv(s, 0, "binv_hash", P_<uint32_t>(s->d_zN), (size_t)n, P_<uint32_t>(s->d_zNi)));
  KL(s, "k_h2c_affine", lsgk::h2c_affine(S_(s), n, P_<uint32_t>(s->d_Hp), P_<uint32_t>(s->d_zNi), hinf, H));
  return LSG_OK;
}

// ---- staging: the package's sets into the slot's pinned arena (order given by `order`),
// randomizers drawn here (seed == 0: OS CSPRNG; else deterministic, for tests).  What is staged
// and how is lsg_stage.hpp's (stage_measure, stage_fill and the meaning of scale, noscale, dedup,
// bits_ok, rnd_in); this is the device side: the buffers sized between the two passes, the copies.
int stage_sets(Slot* s, const lsg_set* const* sets, size_t n, uint64_t seed, bool scale,
               const std::vector<uint8_t>* noscale = nullptr, bool dedup = false, bool bits_ok = false,
               const uint64_t* rnd_in = nullptr) {
  const StageSizes z = stage_measure(sets, n, bits_ok);
  if (z.n_bits_sets + z.n_multi) {
    LSG_RC(ensure_host(s, s->h_cbits, 4 * z.bit_words));
    LSG_RC(ensure(s, s->d_cbits, 4 * z.bit_words));
  }
  LSG_RC(size_inputs(s, n, z.npk, z.msg_total));
  const StageLayout L = stage_layout(n, z.npk, z.pk_stride(), z.msg_total);
  static const bool dedup_on = lsg_ab_long("LSG_MSG_DEDUP", 1) != 0;
  StageOpts o;
  o.scale = scale;
  o.noscale = noscale;
  o.dedup = dedup;
  o.dedup_on = dedup_on;
  o.bits_ok = bits_ok;
  o.rnd_in = rnd_in;
  o.seed = seed;
  const lsg_ctx* c = s->d->c;
  const Committees cm{c->cm_len.data(), c->cm_ok.data(), c->cm_ok.size()};
  uint8_t* A = H_<uint8_t>(s->h_arena);
  uint32_t* cbits = H_<uint32_t>(s->h_cbits);
  // (the message cache: package staging only, s->mc_ok)
  const int rc = stage_fill(A, L, cbits, sets, n, z, o, s->mc_ok ? &s->d->mc : nullptr, cm, s->mtab, s->plan, *s, MsgKey(),
                            os_random);
  if (rc == LSG_ERR_ENTROPY) set_err(s->d->c, "no entropy for the RLC randomizers (getrandom failed)");
  LSG_RC(rc);
  hipStream_t S = s->st[0];
  struct {
    DevBuf* d;
    size_t off, len;
  } cp[] = {{&s->d_sig, L.sig, 192 * L.nn},      {&s->d_siglen, L.siglen, 4 * L.nn},
            {&s->d_msg, L.msg, std::max(s->mc_on ? s->msg_used : z.msg_total, (size_t)1)},
            {&s->d_msgoff, L.msgoff, 4 * L.nn}, {&s->d_msglen, L.msglen, 4 * L.nn}, {&s->d_pk, L.pk, L.stride * L.np},
            {&s->d_pklen, L.pklen, 4 * L.np},   {&s->d_rnd, L.rnd, 8 * L.nn}};
  for (auto& x : cp) LSG_HIP(s, hipMemcpyAsync(x.d->p, A + x.off, x.len, hipMemcpyHostToDevice, S));
  if (s->msg_dedup) LSG_HIP(s, hipMemcpyAsync(s->d_mid.p, A + L.mid, 4 * n, hipMemcpyHostToDevice, S));
  if (s->bit_words) LSG_HIP(s, hipMemcpyAsync(s->d_cbits.p, cbits, 4 * s->bit_words, hipMemcpyHostToDevice, S));
  return LSG_OK;
}

// PublicKey.aggregate of the slot's LSG_PK_BITS sets on the current stream (k_pk_agg_bits; the
// plan s->bplan is in the uploaded arena)
int run_pk_bits(Slot* s, uint32_t* dst) {
  if (s->bits_sets.empty()) return LSG_OK;
  Dev* d = s->d;
  KL(s, "k_pk_agg_bits", lsgk::pk_agg_bits(S_(s), (int)s->bplan.n_pairs, PL(s, s->bplan.pair_off), PL(s, s->bplan.plan_off),
                                           P_<uint32_t>(s->d_cbits), P_<uint32_t>(d->d_cm_idx), P_<uint32_t>(d->d_cm_off),
                                           P_<uint32_t>(d->d_cm_sum), P_<uint32_t>(d->d_pktab), P_<uint8_t>(d->d_pktab_ok),
                                           (uint32_t)d->pktab_n, dst));
  return LSG_OK;
}
// ... and of its LSG_PK_BITS_MULTI sets (k_pk_agg_bits_multi, plan s->mplan): after
// k_pk_agg_bits, into their own slots
int run_pk_multi(Slot* s, uint32_t* dst) {
  if (s->multi_sets.empty()) return LSG_OK;
  Dev* d = s->d;
  KL(s, "k_pk_agg_bits_multi",
     lsgk::pk_agg_bits_multi(S_(s), (int)s->mplan.n_pairs, PL(s, s->mplan.pair_off), PL(s, s->mplan.set_off),
                             PL(s, s->mplan.part_off), P_<uint32_t>(s->d_cbits), P_<uint32_t>(d->d_cm_idx),
                             P_<uint32_t>(d->d_cm_off), P_<uint32_t>(d->d_cm_sum), P_<uint32_t>(d->d_pktab),
                             P_<uint8_t>(d->d_pktab_ok), (uint32_t)d->pktab_n, dst));
  return LSG_OK;
}

// Miller accumulation of planned items (after ev_sig on the main stream)
int launch_accum(Slot* s, size_t n_items, size_t item_off, uint32_t* fall, bool single = false) {
  const int ni = (int)n_items;
  const int32_t* items = PL(s, item_off);
  if (ni > 0 && (single || s->K == 1) && miller_fused() && (size_t)ni <= std::max(slp_items_max(), (size_t)8192) &&
      slp_items_max() > 0) {
    // one-set items (small packages, per-job fallback phases): straight-line programs
    KL(s, "k_slp_items1", lsg_slp_miller_items1(S_(s), ni, items, P_<uint32_t>(s->d_P), P_<uint8_t>(s->d_pinf),
                                                P_<uint8_t>(s->d_hinf), P_<int32_t>(s->d_seterr), P_<uint32_t>(s->d_H),
                                                fall));
    return LSG_OK;
  }
  if (single && ni > 0) {
    // every item is one pair (a fallback phase of single-set jobs): the fused kernel would run
    // four waves per item for one pair; the list form computes each set's lines once and
    // accumulates them alone (item k = set items[k])
    LSG_RC(ensure(s, s->d_lines, 4 * (size_t)ML_STEPS * W_LINE * n_items));
    KL(s, "k_miller_lines_list", lsgk::miller_lines_list(S_(s), ni, items, P_<uint32_t>(s->d_H), P_<uint32_t>(s->d_lines)));
    KL(s, "k_miller_accum_list",
       lsgk::miller_accum_list(S_(s), ni, items, P_<uint32_t>(s->d_P), P_<uint8_t>(s->d_pinf), P_<uint8_t>(s->d_hinf),
                               P_<int32_t>(s->d_seterr), P_<uint32_t>(s->d_lines), fall));
    return LSG_OK;
  }
  if (miller_fused()) {
    if (mf_lanes_on())
      KL(s, "k_miller_fused", lsgk::miller_fused(S_(s), ni, items, items + ni, P_<uint32_t>(s->d_P), P_<uint8_t>(s->d_pinf),
                                                P_<uint8_t>(s->d_hinf), P_<int32_t>(s->d_seterr), P_<uint32_t>(s->d_H),
                                                fall));
    else
      KL(s, "k_miller_fused_pair",
         lsgk::miller_fused(S_(s), ni, items, items + ni, P_<uint32_t>(s->d_P), P_<uint8_t>(s->d_pinf),
                            P_<uint8_t>(s->d_hinf), P_<int32_t>(s->d_seterr), P_<uint32_t>(s->d_H), fall, true));
    return LSG_OK;
  }
  KL(s, "k_miller_accum",
     lsgk::miller_accum(S_(s), s->K, ni, items, items + ni, P_<uint32_t>(s->d_P), P_<uint8_t>(s->d_pinf),
                        P_<uint8_t>(s->d_hinf), P_<int32_t>(s->d_seterr), (int)s->n_sets, P_<uint32_t>(s->d_lines),
                        fall));
  return LSG_OK;
}

// The bucket sums of the phase's MSM groups: the first pass folds the resident affine signatures
// themselves (lsg_k_sig.hip k_msm_bucket_seg on plan_buckets' plan), buckets longer than a chunk
// finish through k_seg_reduce<1>; compare run_pk_seg.  LSG_MSM_FOLD=0 (A/B build): the passes of
// plan_seg over the projective copies in rs_msm (k_sig_proj).
int run_msm_buckets(Slot* s, const SegPlan& P, const uint32_t* rs_msm, uint32_t* dst) {
  if (!s->sw.msm_fold) return run_seg(s, 1, "msm_buckets", P, rs_msm, dst);
  LSG_RC(size_seg(s, 1, P));
  uint32_t* tmp[3] = {nullptr, P_<uint32_t>(s->seg_tmp[1][0]), P_<uint32_t>(s->seg_tmp[1][1])};
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    if (k == 0)
      KL(s, "msm_buckets", lsgk::msm_bucket_seg(S_(s), q.n_chunks, q.ips_log2, PL(s, q.chunk_off), PL(s, P.idx_off),
                                                P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                                P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), dst, tmp[q.tmp_out],
                                                !fp2_lanes_on()));
    else
      KL(s, "msm_buckets", lsgk::seg_reduce(S_(s), 1, q.n_chunks, q.ips_log2, PL(s, q.chunk_off), nullptr, tmp[q.src],
                                            dst, tmp[q.tmp_out]));
  }
  return LSG_OK;
}

// side stream: signature sums -> ML(-G1, S_g) -> fall slots; main stream: products, export, FE
// rs: the scaled points [r_i] sig_i the plain groups sum; rs_msm: the unscaled points the
// bucket MSM groups read where their bucket pass reads projective copies (LSG_MSM_FOLD=0; phase
// A: one buffer holds both kinds, by set) -- the shipped bucket pass reads d_sigaff itself
int launch_phase(Slot* s, const PhasePlan& Ph, const uint32_t* rs, uint32_t* fall, bool export_blobs,
                 const uint32_t* rs_msm = nullptr) {
  if (!rs_msm) rs_msm = rs;
  const size_t ng = Ph.groups.size();
  if (ng == 0) return LSG_OK;
  LSG_RC(size_state(s, s->n_sets, s->n_pks, ng, Ph.n_msm, 2));
  s->cur = 1;
  if (Ph.n_msm) {
    LSG_RC(run_msm_buckets(s, Ph.buckets, rs_msm, P_<uint32_t>(s->d_bkt)));
    LSG_RC(run_seg(s, 1, "msm_bits", Ph.bits, P_<uint32_t>(s->d_bkt), P_<uint32_t>(s->d_bits)));
    KL(s, "k_g2p_to_canon", lsgk::g2p_to_canon(S_(s), (int)(MSM_BITS * Ph.n_msm), P_<uint32_t>(s->d_bits),
                                               P_<uint8_t>(s->d_Sb)));
    KL(s, "slp_horner_miller",
       lsg_slp_horner_miller(S_(s), (int)Ph.n_msm, P_<uint8_t>(s->d_Sb), P_<uint8_t>(s->d_fgb)));
  }
  if (Ph.n_msm < ng) {
    const int nsm = (int)(ng - Ph.n_msm);
    LSG_RC(run_seg(s, 1, "sig_sums", Ph.sums, rs, P_<uint32_t>(s->d_S)));
    uint8_t* sb = P_<uint8_t>(s->d_Sb) + (size_t)288 * MSM_BITS * Ph.n_msm;
    KL(s, "k_g2p_to_canon", lsgk::g2p_to_canon(S_(s), nsm, P_<uint32_t>(s->d_S) + W_G2P * Ph.n_msm, sb));
    KL(s, "slp_miller_neg_g1",
       lsg_slp_miller_neg_g1(S_(s), nsm, sb, P_<uint8_t>(s->d_fgb) + 576 * Ph.n_msm));
  }
  KL(s, "k_blobs_to_fp12", lsgk::blobs_to_fp12(S_(s), (int)ng, P_<uint8_t>(s->d_fgb), fall + W_F12 * Ph.term_base));
  LSG_HIP(s, hipEventRecord(s->ev_grp, s->st[1]));
  s->cur = 0;
  LSG_HIP(s, hipStreamWaitEvent(s->st[0], s->ev_grp, 0));
  LSG_RC(run_seg(s, 2, "fp12_product", Ph.prod, fall, P_<uint32_t>(s->d_F)));
  KL(s, "k_fp12_to_canon", lsgk::fp12_to_canon(S_(s), (int)ng, P_<uint32_t>(s->d_F), P_<uint8_t>(s->d_Fb)));
  if (export_blobs) LSG_HIP(s, hipMemcpyAsync(s->h_blob.p, s->d_Fb.p, 576 * ng, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipEventRecord(s->ev_part, s->st[0]));
  return LSG_OK;
}

// FE of the phase's groups g0 .. g1-1 + verdict readback (main stream)
int launch_fe_range(Slot* s, size_t g0, size_t g1) {
  if (g1 <= g0) return LSG_OK;
  s->cur = 0;
  const size_t ng = g1 - g0;
  KL(s, "slp_final_exp",
     lsg_slp_final_exp(S_(s), (int)ng, P_<uint8_t>(s->d_Fb) + 576 * g0, P_<int32_t>(s->d_verdict) + g0));
  LSG_HIP(s, hipMemcpyAsync(H_<int32_t>(s->h_verdict) + g0, P_<int32_t>(s->d_verdict) + g0, 4 * ng,
                            hipMemcpyDeviceToHost, s->st[0]));
  return LSG_OK;
}
int launch_fe(Slot* s, size_t ng) { return launch_fe_range(s, 0, ng); }

int launch_agg_tree(Slot* s, const AggPlan& P, uint32_t* agg);

// Per-set stages of the slot's package (no host synchronisation):
//   side: pubkeys -> aggregation -> [r_i] scaling -> signature decode -> subgroup check (ev_sig)
//   main: expand_message -> hash_to_G2 [-> lines] -> wait ev_sig -> Miller items f (fall)
int launch_set_stages(Slot* s, const SegPlan* pkagg, const PhasePlan& Ph, uint32_t* fall) {
  const size_t n_items = Ph.agg_g >= 0 ? Ph.n_set_items : Ph.n_items, item_off = Ph.item_off;
  const int n = (int)s->n_sets, np = (int)s->n_pks;
  if (n == 0) return LSG_OK;
  Dev* d = s->d;
  LSG_HIP(s, hipEventRecord(s->ev_in, s->st[0]));
  s->cur = 1;
  LSG_HIP(s, hipStreamWaitEvent(s->st[1], s->ev_in, 0));
  if (!s->single_keys && s->agg.tree) {
    LSG_RC(launch_agg_tree(s, s->agg, P_<uint32_t>(s->d_agg)));
  } else if (s->single_keys) {
    // single-key sets decode straight into their aggregate slot
    if (np > 0)
      KL(s, "k_pk_decode", lsgk::pk_decode(S_(s), np, P_<uint8_t>(s->d_pk), s->pk_stride, P_<uint32_t>(s->d_pklen),
                                           P_<uint32_t>(s->d_agg), P_<int32_t>(s->d_pkerr), P_<uint32_t>(d->d_pktab),
                                           P_<uint8_t>(d->d_pktab_ok), (uint32_t)d->pktab_n));
  } else if (!s->pk_all_bits) {
    LSG_RC(run_pk_seg(s, *pkagg, P_<uint32_t>(s->d_agg)));  // (every staged key is in one set)
  }
  // committee + bits sets: their aggregates over whatever run_pk_seg left in their slots (the
  // identity of a set without staged keys)
  LSG_RC(run_pk_bits(s, P_<uint32_t>(s->d_agg)));
  LSG_RC(run_pk_multi(s, P_<uint32_t>(s->d_agg)));
  // flagged jobs' byte keys: KeyValidate codes per list item (d_pkp is free in a package: the
  // keys decode straight into their aggregates); applied to the sets after the signature stages
  if (s->n_kv)
    KL(s, "k_pk_keyvalidate", lsgk::pk_keyvalidate(S_(s), (int)s->n_kv, PL(s, s->kv_off), P_<uint8_t>(s->d_pk),
                                                   P_<uint32_t>(s->d_pklen), P_<int32_t>(s->d_pkp)));
  KL(s, "k_pk_scale", lsgk::pk_scale(S_(s), n, P_<uint32_t>(s->d_agg), P_<uint64_t>(s->d_rnd), P_<uint32_t>(s->d_Pp),
                                     P_<uint32_t>(s->d_zP), P_<uint8_t>(s->d_pinf)));
  LSG_RC(batch_inv(s, 1, "binv_pk", P_<uint32_t>(s->d_zP), (size_t)n, P_<uint32_t>(s->d_zPi)));
  KL(s, "k_pk_affine", lsgk::pk_affine(S_(s), n, P_<uint32_t>(s->d_Pp), P_<uint32_t>(s->d_zPi), P_<uint32_t>(s->d_P)));
  const lsgk::PowLanes pw = pow_lanes(s->d_pwsig, (size_t)n, lsgk::POW_SIG_STATE);
  KL(s, "k_sig_decode", lsgk::sig_decode(S_(s), n, P_<uint8_t>(s->d_sig), P_<uint32_t>(s->d_siglen),
                                         P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf), P_<int32_t>(s->d_seterr), pw));
  KL_POW(s, pw, n);
  if ((size_t)n <= slp_items_max())  // small packages: one program per set (0.3 ms, not 1.3)
    KL(s, "k_slp_subgroup", lsg_slp_g2_subgroup(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                                P_<int32_t>(s->d_seterr)));
  else
    LSG_RC(launch_sig_subgroup(s, n));
  if (s->n_kv)  // a key error beats a signature error (the reference validates the key first)
    KL(s, "k_pk_keyvalidate_apply", lsgk::pk_keyvalidate_apply(S_(s), (int)s->n_kv, PL(s, s->kv_off + s->n_kv),
                                                               P_<int32_t>(s->d_pkp), P_<int32_t>(s->d_seterr)));
  if (Ph.agg_g >= 0) {  // per message: sum of the package group's usable r_i pk_i, affine
    const Grp& g = Ph.groups[(size_t)Ph.agg_g];
    const size_t nm = Ph.n_magg;
    LSG_RC(ensure(s, s->d_mmask, 4 * W_G1P * std::max(g.first + g.len, (size_t)1)));
    LSG_RC(ensure(s, s->d_PmP, 4 * W_G1P * nm));
    LSG_RC(ensure(s, s->d_Pm, 4 * W_G1A * nm));
    LSG_RC(ensure(s, s->d_pinfm, nm));
    LSG_RC(ensure(s, s->d_errm, 4 * nm));
    KL(s, "k_pk_mask", lsgk::pk_mask(S_(s), (int)(g.first + g.len), P_<uint32_t>(s->d_Pp), P_<int32_t>(s->d_seterr),
                                     P_<uint8_t>(s->d_pinf), P_<uint32_t>(s->d_mmask)));
    LSG_RC(run_seg(s, 0, "msg_pk_sums", s->msum, P_<uint32_t>(s->d_mmask), P_<uint32_t>(s->d_PmP)));
    KL(s, "k_g1p_affine_inv", lsgk::g1p_affine_inv(S_(s), (int)nm, P_<uint32_t>(s->d_PmP), P_<uint32_t>(s->d_Pm),
                                                   P_<uint8_t>(s->d_pinfm)));
    LSG_HIP(s, hipMemsetAsync(s->d_errm.p, 0, 4 * nm, s->st[1]));
  }
  LSG_HIP(s, hipEventRecord(s->ev_sig, s->st[1]));
  s->cur = 0;
  // hash_to_G2 once per distinct message, then each set's point gathered from its message's
  const int nm = (int)s->n_msgs;
  if (s->mc_on && (s->mc_hits || !s->mc_pend.empty())) {
    // the message cache: only the nx misses are staged and hashed (none: no hash-stage kernel
    // runs); with a hit among the messages they go to d_Hx and k_h2c_cache_merge fills the
    // per-message (or, every set its own message, per-set) points from rows and misses
    const int nx = (int)s->n_miss;
    const bool merge = s->mc_hits > 0;
    uint32_t* Hd = P_<uint32_t>(s->d_H);
    uint8_t* hd = P_<uint8_t>(s->d_hinf);
    if (s->msg_dedup) {
      LSG_RC(ensure(s, s->d_Hm, 4 * W_G2A * (size_t)nm));
      LSG_RC(ensure(s, s->d_hinfm, (size_t)nm));
      Hd = P_<uint32_t>(s->d_Hm);
      hd = P_<uint8_t>(s->d_hinfm);
    }
    uint32_t* Hx = Hd;
    uint8_t* hx = hd;
    if (merge) {
      LSG_RC(ensure(s, s->d_Hx, 4 * W_G2A * (size_t)std::max(nx, 1)));
      LSG_RC(ensure(s, s->d_hinfx, (size_t)std::max(nx, 1)));
      Hx = P_<uint32_t>(s->d_Hx);
      hx = P_<uint8_t>(s->d_hinfx);
    }
    if (nx > 0) {
      if (s->msg_objs)
        KL(s, "k_msg_roots", lsgk::msg_roots(S_(s), nx, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                             P_<uint32_t>(s->d_msglen)));
      if (s->msg_vars)
        KL(s, "k_msg_roots_var", lsgk::msg_roots_var(S_(s), nx, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                                     P_<uint32_t>(s->d_msglen), nullptr));
      KL(s, "k_expand_msg", lsgk::expand_msg(S_(s), nx, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                             P_<uint32_t>(s->d_msglen), P_<uint8_t>(s->d_dst), DST_POP_LEN,
                                             P_<uint8_t>(s->d_ub)));
      LSG_RC(launch_hash(s, nx, Hx, hx));
    }
    const uint32_t n_rows = d->mc.capacity();
    if (merge)
      KL(s, "k_h2c_cache_merge",
         lsgk::h2c_cache_merge(S_(s), nm, (const uint32_t*)PL(s, s->mc_src_off), n_rows, P_<uint32_t>(d->d_mc_rows),
                               P_<uint8_t>(d->d_mc_inf), (uint32_t)nx, Hx, hx, Hd, hd));
    if (!s->mc_pend.empty())
      KL(s, "k_h2c_cache_store",
         lsgk::h2c_cache_store(S_(s), (int)s->mc_pend.size(), (const uint32_t*)PL(s, s->mc_st_off), (uint32_t)nx, Hx, hx,
                               n_rows, P_<uint32_t>(d->d_mc_rows), P_<uint8_t>(d->d_mc_inf)));
    if (s->msg_dedup)
      KL(s, "k_h2c_gather", lsgk::h2c_gather(S_(s), n, P_<uint32_t>(s->d_mid), P_<uint32_t>(s->d_Hm),
                                             P_<uint8_t>(s->d_hinfm), P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf)));
  } else {
    if (s->msg_objs)  // LSG_MSG_OBJECT messages: object + domain -> the 32-byte signing root, in place
      KL(s, "k_msg_roots", lsgk::msg_roots(S_(s), nm, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                           P_<uint32_t>(s->d_msglen)));
    if (s->msg_vars)  // tagged messages (AggregateAndProof): one workgroup each, likewise in place
      KL(s, "k_msg_roots_var", lsgk::msg_roots_var(S_(s), nm, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                                   P_<uint32_t>(s->d_msglen), nullptr));
    KL(s, "k_expand_msg", lsgk::expand_msg(S_(s), nm, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                           P_<uint32_t>(s->d_msglen), P_<uint8_t>(s->d_dst), DST_POP_LEN,
                                           P_<uint8_t>(s->d_ub)));
    if (s->msg_dedup) {
      LSG_RC(ensure(s, s->d_Hm, 4 * W_G2A * (size_t)nm));
      LSG_RC(ensure(s, s->d_hinfm, (size_t)nm));
      LSG_RC(launch_hash(s, nm, P_<uint32_t>(s->d_Hm), P_<uint8_t>(s->d_hinfm)));
      KL(s, "k_h2c_gather", lsgk::h2c_gather(S_(s), n, P_<uint32_t>(s->d_mid), P_<uint32_t>(s->d_Hm),
                                             P_<uint8_t>(s->d_hinfm), P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf)));
    } else {
      LSG_RC(launch_hash(s, n, P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf)));
    }
  }
  if (!miller_fused())
    KL(s, "k_miller_lines", lsgk::miller_lines(S_(s), n, P_<uint32_t>(s->d_H), P_<uint32_t>(s->d_lines)));
  LSG_HIP(s, hipStreamWaitEvent(s->st[0], s->ev_sig, 0));
  if (n_items) LSG_RC(launch_accum(s, n_items, item_off, fall));
  if (Ph.agg_g >= 0)  // one pair per message: (sum of r_i pk_i, H(m)), one program each
    KL(s, "k_slp_items_msg",
       lsg_slp_miller_items1(S_(s), (int)Ph.n_magg, PL(s, Ph.magg_off), P_<uint32_t>(s->d_Pm), P_<uint8_t>(s->d_pinfm),
                             P_<uint8_t>(s->d_hinfm), P_<int32_t>(s->d_errm), P_<uint32_t>(s->d_Hm),
                             fall + (size_t)lsgl::W_F12 * Ph.n_set_items));
  return LSG_OK;
}

// pubkey aggregation plan (sets with several keys): segment i = keys pk_first[i] ..
SegPlan plan_pk_agg(Slot* s) {
  std::vector<int32_t> off(s->n_sets), len(s->n_sets);
  for (size_t i = 0; i < s->n_sets; i++) {
    off[i] = (int32_t)s->shape.pk_first[i];
    len[i] = (int32_t)s->shape.pk_cnt[i];
  }
  return slot_seg(s, 0, off, len, false, 0, 0);
}

// The batch-affine tree's plan for the slot's sets (keys of set i: pk_first[i] .. + pk_cnt[i]).
// L is chosen by cost: a tree set of n keys costs ~7 products per level-0 point (padded to
// 2^L: one fold product, five in the step, a share of the heaps) plus 11 per complete mixed
// addition of its ceil(n / 2^L) level-L points; a set the tree would not make cheaper (few
// keys, or padding too large) is summed from its keys directly by k_agg_final.
AggPlan plan_agg_tree(Slot* s) {
  AggPlan P;
  P.tree = true;
  const size_t n = s->n_sets;
  auto tree_cost = [](int64_t len, int L) {
    const int64_t A = (int64_t)1 << L;
    return ((len + A - 1) / A) * A * 7 + ((len + A - 1) / A) * 11;
  };
  int64_t best = -1;
  for (int L = 0; L <= 9; L++) {
    int64_t cost = 0;
    for (size_t i = 0; i < n; i++) {
      const int64_t len = (int64_t)s->shape.pk_cnt[i];
      cost += L > 0 ? std::min(tree_cost(len, L), len * 11) : len * 11;
    }
    if (best < 0 || cost < best) {
      best = cost;
      P.L = L;
    }
  }
  const int64_t A = (int64_t)1 << P.L;
  P.T = (int)std::max<long>(1, std::min<long>(64, lsg_ab_long("LSG_AGG_T", 8)));
  std::vector<int32_t> o0(n, 0), src(3 * n);
  int64_t N0 = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t len = (int64_t)s->shape.pk_cnt[i];
    if (P.L > 0 && tree_cost(len, P.L) < len * 11) {
      o0[i] = (int32_t)N0;
      src[3 * i] = 0;
      src[3 * i + 1] = (int32_t)(N0 >> P.L);
      src[3 * i + 2] = (int32_t)((len + A - 1) / A);
      N0 += (len + A - 1) / A * A;
    } else {
      src[3 * i] = 1;
      src[3 * i + 1] = (int32_t)s->shape.pk_first[i];
      src[3 * i + 2] = (int32_t)len;
    }
  }
  P.N0 = N0;
  if (N0 == 0) P.L = 0;
  if (P.L > 0) {
    // lane pairs: a multiple of 128 << (L - 1), so that every level's grid is whole blocks
    const int64_t unit = (int64_t)LSG_ITEMS_PER_BLOCK_HOST << (P.L - 1);
    const int64_t need = (N0 / 2 + P.T - 1) / P.T;
    P.n_c0 = (need + unit - 1) / unit * unit;
    P.blk_off = s->plan.size();
    s->plan.resize(P.blk_off + (size_t)(N0 >> P.L));
    int32_t* blk = s->plan.data() + P.blk_off;
    for (size_t i = 0; i < n; i++)
      if (src[3 * i] == 0)
        for (int32_t b = src[3 * i + 1], e = b + src[3 * i + 2]; b < e; b++) blk[b] = (int32_t)i;
  }
  P.o0_off = s->plan.size();
  s->plan.insert(s->plan.end(), o0.begin(), o0.end());
  P.len_off = s->plan.size();
  for (size_t i = 0; i < n; i++) s->plan.push_back((int32_t)s->shape.pk_cnt[i]);
  P.pk0_off = s->plan.size();
  for (size_t i = 0; i < n; i++) s->plan.push_back((int32_t)s->shape.pk_first[i]);
  P.src_off = s->plan.size();
  s->plan.insert(s->plan.end(), src.begin(), src.end());
  return P;
}

// the tree over the staged keys into d_agg (side stream: after the inputs' upload)
int launch_agg_tree(Slot* s, const AggPlan& P, uint32_t* agg) {
  Dev* d = s->d;
  lsgk::AggTreeArgs a;
  a.L = P.L;
  a.T = P.T;
  a.n_c0 = P.n_c0;
  a.N0 = P.N0;
  a.blk_set = PL(s, P.blk_off);
  a.set_o0 = PL(s, P.o0_off);
  a.set_len = PL(s, P.len_off);
  a.set_pk0 = PL(s, P.pk0_off);
  a.pk = P_<uint8_t>(s->d_pk);
  a.stride = s->pk_stride;
  a.pk_len = P_<uint32_t>(s->d_pklen);
  a.pk_err = P_<int32_t>(s->d_pkerr);
  a.tab = P_<uint32_t>(d->d_pktab);
  a.tab_ok = P_<uint8_t>(d->d_pktab_ok);
  a.tab_n = (uint32_t)d->pktab_n;
  if (P.L > 0) {
    const size_t npts = (size_t)(2 * P.N0), pre_w = W_FP * (size_t)(P.T * P.n_c0), cinv_w = W_FP * (size_t)P.n_c0;
    LSG_RC(ensure(s, s->d_agga, 4 * W_G1A * npts));
    LSG_RC(ensure(s, s->d_aggi, npts));
    LSG_RC(ensure(s, s->d_aggpre, 4 * 2 * pre_w));
    LSG_RC(ensure(s, s->d_aggtot, 4 * 2 * cinv_w));
    LSG_RC(ensure(s, s->d_aggflag, 2 * (size_t)P.n_c0));
    a.pts = P_<uint32_t>(s->d_agga);
    a.inf = P_<uint8_t>(s->d_aggi);
    a.pre[0] = P_<uint32_t>(s->d_aggpre);
    a.pre[1] = a.pre[0] + pre_w;
    a.cinv[0] = P_<uint32_t>(s->d_aggtot);
    a.cinv[1] = a.cinv[0] + cinv_w;
    a.flag[0] = P_<uint8_t>(s->d_aggflag);
    a.flag[1] = a.flag[0] + P.n_c0;
    KL(s, "g1_aggregate", lsgk::agg_leaf(S_(s), a));
    for (int t = 0; t < P.L; t++) KL(s, "g1_aggregate", lsgk::agg_step(S_(s), a, t));
  }
  KL(s, "g1_aggregate", lsgk::agg_final(S_(s), a, (int)s->n_sets, PL(s, P.src_off), agg));
  return LSG_OK;
}

// D2H of per-set status into the pinned mirrors, then ev_done on the main stream
int launch_readback(Slot* s, bool status) {
  hipStream_t S = s->st[0];
  const size_t n = s->n_sets, np = s->n_pks;
  if (s->own_streams) {  // join the side stream
    LSG_HIP(s, hipEventRecord(s->ev_grp, s->st[1]));
    LSG_HIP(s, hipStreamWaitEvent(S, s->ev_grp, 0));
  }
  if (status) {
    if (n) {
      LSG_HIP(s, hipMemcpyAsync(s->h_err.p, s->d_seterr.p, 4 * n, hipMemcpyDeviceToHost, S));
      LSG_HIP(s, hipMemcpyAsync(s->h_pinf.p, s->d_pinf.p, n, hipMemcpyDeviceToHost, S));
    }
    if (np) LSG_HIP(s, hipMemcpyAsync(s->h_pkerr.p, s->d_pkerr.p, 4 * np, hipMemcpyDeviceToHost, S));
  }
  LSG_HIP(s, hipEventRecord(s->ev_done, S));
  return LSG_OK;
}

SetStatus read_status(Slot* s) {
  SetStatus ss;
  const size_t n = s->n_sets;
  ss.err = H_<int32_t>(s->h_err);
  ss.pkerr = H_<int32_t>(s->h_pkerr);
  ss.pinf.assign(H_<uint8_t>(s->h_pinf), H_<uint8_t>(s->h_pinf) + n);
  for (size_t i = 0; i < n; i++)
    if (s->shape.pk_cnt[i] == 0 && !(i < s->shape.bits_p.size() && s->shape.bits_p[i] > 0))
      ss.pinf[i] = 2;  // PublicKey.aggregate([]) throws (a bits set: no participant)
  return ss;
}

}  // namespace

// ---------------------------------------------------------------------------- packages
namespace {

const uint8_t* fp12_one_blob() {  // canonical Fp12 one: c0.c0.c0 = 1
  static uint8_t b[576] = {0};
  b[47] = 1;
  return b;
}

// sig_prep into `out` for the slot's sets on the side stream.  mode: per-set bytes (1 =
// scale) or null; rnd null = no scaling at all (every group sums by the bucket MSM).
int launch_sig_prep(Slot* s, bool scale, const std::vector<uint8_t>* mode, uint32_t* out) {
  const int n = (int)s->n_sets;
  if (n == 0) return LSG_OK;
  s->cur = 1;
  const uint8_t* dm = nullptr;
  if (scale && mode) {
    LSG_RC(ensure_host(s, s->h_mode, (size_t)n));
    LSG_RC(ensure(s, s->d_mode, (size_t)n));
    memcpy(s->h_mode.p, mode->data(), (size_t)n);
    LSG_HIP(s, hipMemcpyAsync(s->d_mode.p, s->h_mode.p, (size_t)n, hipMemcpyHostToDevice, s->st[1]));
    dm = P_<uint8_t>(s->d_mode);
  }
  if (scale && (size_t)n <= slp_items_max()) {
    // small packages: the unscaled points, then [r_i] sig_i as one program per scaled set
    // (0.45 ms instead of a 64-bit scalar multiplication per lane pair, 2.2 ms)
    KL(s, "k_sig_prep", lsgk::sig_prep(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                       P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), nullptr, nullptr, out));
    KL(s, "k_slp_g2_scale", lsg_slp_g2_scale(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                             P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), P_<uint64_t>(s->d_rnd),
                                             dm, out));
    return LSG_OK;
  }
  KL(s, "k_sig_prep", lsgk::sig_prep(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                     P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf),
                                     scale ? P_<uint64_t>(s->d_rnd) : nullptr, dm, out));
  return LSG_OK;
}

// Part 1 of phase A on one device: stage this device's jobs (ids into `jobs`; batchable jobs
// first), plan and launch every per-set stage and group stage up to the canonical products
// (ev_part).  n_node > 0: this slot also reduces the all-gathered partials of n_node devices
// (its plan holds that product's chunk list).
// lone_ok: a set alone in its phase-A group may be verified unscaled (a plain verify, as
// maybeBatch.ts:34-38).  False when the package group's partial is multiplied with other
// partials before its verdict (a multi-device ticket, lsg_batch_partial): there every r_i is
// random and nonzero, or two forged one-set shards (sig_a + D, sig_b - D) would pass together.
// dev_msgs: the sets' 32-byte messages are already on this device, one per staged set in
// staging order (lsg_verify_deposits: the signing roots never leave the GPU); the sets' host
// msg bytes are placeholders then and are overwritten by a device copy.
int pkg_part1(Slot* s, const lsg_job* jobs, const std::vector<size_t>& ids, uint64_t seed, int n_node,
              const std::vector<size_t>* subs = nullptr, bool lone_ok = true, const uint8_t* dev_msgs = nullptr,
              const uint32_t* set_group = nullptr, size_t n_groups = 0, const uint64_t* rnd_in = nullptr,
              bool msg_cache = true) {
  timer_reset(s);
  s->plan.clear();
  memset(&s->stats, 0, sizeof(s->stats));
  s->stats.start_ns = now_ns();
  const size_t nj = ids.size();
  s->results.assign(nj, lsg_job_result{LSG_INVALID, 0});
  s->rs2_ready = false;
  s->rs2_scaled.clear();
  s->has_node = n_node > 0;
  s->big_fe_pending = false;
  s->seed = seed;
  s->resolved = s->resolving = false;
  s->resolve_rc = LSG_OK;
  std::vector<const lsg_set*> flat(shape_jobs(s->shape, jobs, ids, subs));
  for (size_t k = 0; k < nj; k++)
    for (uint32_t q = 0; q < jobs[ids[k]].n_sets; q++) flat[s->shape.jobs[k].first + q] = &jobs[ids[k]].sets[q];
  // a grouped package (single device: ids ascend): the caller's group word of every staged set
  s->grp_n = set_group ? n_groups : 0;
  if (s->grp_n) {
    s->set_grp.assign(flat.size(), LSG_NO_GROUP);
    size_t j = 0, before = 0;
    for (size_t k = 0; k < nj; k++) {
      for (; j < ids[k]; j++) before += jobs[j].n_sets;
      for (uint32_t q = 0; q < jobs[ids[k]].n_sets; q++) s->set_grp[s->shape.jobs[k].first + q] = set_group[before + q];
    }
  }
  if (subs) {  // a coalesced launch: per-sub state
    lsg_stats z;
    memset(&z, 0, sizeof(z));
    s->sub_stats.assign(s->shape.n_sub, z);
    s->sub_pkfail.assign(s->shape.n_sub, 0);
    s->sub_done.assign(s->shape.n_sub, 0);
  }
  s->K = miller_k_for(flat.size());
  // phase-A groups, MSM groups first: the package group (a coalesced launch: one per
  // sub-package, each with its own verdicts, chunks and fallback), then the non-batchable jobs
  s->sw = read_switches();
  s->gp = plan_groups(s->shape, s->sw, lone_ok);
  const uint64_t th0 = trace_host() ? now_ns() : 0;
  s->mc_ok = msg_cache;  // (only here: every other caller of stage_sets stays outside the message cache)
  const int src = stage_sets(s, flat.data(), flat.size(), seed, true, &s->gp.noscale, dev_msgs == nullptr, true, rnd_in);
  s->mc_ok = false;
  LSG_RC(src);
  if (dev_msgs && !flat.empty())  // (placeholders are never merged: message i is set i's)
    LSG_HIP(s, hipMemcpyAsync(s->d_msg.p, dev_msgs, 32 * flat.size(), hipMemcpyDeviceToDevice, s->st[0]));
  // the byte keys of LSG_JOB_VALIDATE_KEYS jobs, compacted
  s->n_kv = plan_validate_keys(s->shape, flat.data(), flat.size(), s->plan, &s->kv_off);
  const uint64_t th1 = trace_host() ? now_ns() : 0;
  PhasePlan& A = s->phA;
  A = PhasePlan();
  A.groups = s->gp.groups;
  A.sub = s->gp.sub;
  size_t n_msm = 0;
  while (n_msm < A.groups.size() && A.groups[n_msm].msm) n_msm++;
  LSG_RC(size_state(s, s->n_sets, s->n_pks, A.groups.size(), n_msm, 1));
  s->agg = AggPlan();
  if (!s->single_keys && !s->pk_all_bits) {
    if (s->n_pks >= AGG_TREE_MIN_KEYS && agg_tree_on() && s->bits_sets.empty() && s->multi_sets.empty())
      s->agg = plan_agg_tree(s);
    else
      s->pkagg = plan_pk_agg(s);
  }
  s->bplan = plan_bits(s->plan, s->bits_sets);
  s->mplan = plan_multi(s->plan, s->multi_sets, s->multi_parts);
  // sets of the package group that share a message share one Miller pair: Π e(r_i pk_i, H(m))
  // = e(Σ r_i pk_i, H(m)) exactly.  Its per-set items are then never computed, so a failing
  // package group's chunks (phase B) run their own items and phase C goes per job.
  A.agg_g = -1;
  if (s->msg_dedup && !s->gp.chunk_mode && s->gp.big_g >= 0 && s->sw.msg_agg && s->n_msgs <= (size_t)8192 &&
      s->sw.slp_items > 0) {
    s->msum = plan_msg_lists(s->plan, s->msg_id.data(), s->n_msgs, A.groups[(size_t)s->gp.big_g], s->sw.seg_fold_wide);
    A.agg_g = s->gp.big_g;
    A.n_magg = s->n_msgs;
  }
  plan_phase(s->plan, s->rnd, s->K, s->sw, A);
  group_items(s->gp, s->shape, A);
  SegPlan node;
  if (n_node > 0) {
    std::vector<int32_t> off{0}, len{(int32_t)n_node};
    node = slot_seg(s, 2, off, len, false, 0, 0);
  }
  LSG_RC(upload_plan(s));
  const uint64_t th2 = trace_host() ? now_ns() : 0;
  LSG_RC(launch_set_stages(s, &s->pkagg, A, P_<uint32_t>(s->d_fall)));
  const uint64_t th3 = trace_host() ? now_ns() : 0;
  // signature points: [r_i] sig_i for the groups that sum scaled points; the MSM groups' bucket
  // pass reads the affine signatures, so a package of MSM groups alone prepares none (rs_raw: the
  // set was in an MSM group here, so a fallback group of such sets may run its own bucket MSM)
  s->rs_raw.assign(s->n_sets, 0);
  for (size_t g = 0; g < A.n_msm; g++) memset(s->rs_raw.data() + A.groups[g].first, 1, A.groups[g].len);
  if (!A.groups.empty()) {
    const bool any_small = A.n_msm < A.groups.size();
    std::vector<uint8_t> mode;
    if (any_small && A.n_msm) {
      mode.assign(s->n_sets, 0);
      for (size_t g = A.n_msm; g < A.groups.size(); g++)
        memset(mode.data() + A.groups[g].first, 1, A.groups[g].len);
    }
    if (any_small || !s->sw.msm_fold)
      LSG_RC(launch_sig_prep(s, any_small, mode.empty() ? nullptr : &mode, P_<uint32_t>(s->d_rs)));
  }
  LSG_RC(launch_phase(s, A, P_<uint32_t>(s->d_rs), P_<uint32_t>(s->d_fall), true));
  if (A.groups.empty() || s->gp.big_g < 0) {  // no package group: the partial is the identity
    s->cur = 0;
    LSG_HIP(s, hipMemcpyAsync(P_<uint8_t>(s->d_gath) + 576 * LSG_MAX_DEVICES, fp12_one_blob(), 576,
                              hipMemcpyHostToDevice, s->st[0]));
    LSG_HIP(s, hipEventRecord(s->ev_part, s->st[0]));
  }
  // the group sums over every grouped set, at the end of the side stream's work (beside the
  // Miller products and final exponentiations on the main stream; launch_readback joins it)
  const uint64_t th4 = trace_host() ? now_ns() : 0;
  if (s->grp_n) {
    s->cur = 1;
    LSG_RC(run_sig_groups(s, nullptr));
    s->cur = 0;
  }
  s->phA_node = node;
  if (trace_host()) {
    fprintf(stderr, "lsg host: sets %zu jobs %zu subs %d groups %zu | stage %.3f plan %.3f set-launch %.3f group-launch %.3f ms",
            (size_t)s->n_sets, nj, s->shape.n_sub, A.groups.size(), (th1 - th0) * 1e-6, (th2 - th1) * 1e-6, (th3 - th2) * 1e-6,
            (th4 - th3) * 1e-6);
    if (s->grp_n) fprintf(stderr, " sig-groups %.3f ms", (now_ns() - th4) * 1e-6);
    fprintf(stderr, "\n");
  }
  return LSG_OK;
}

// device pointer of the package group's canonical partial (576 bytes)
const uint8_t* pkg_partial_dev(Slot* s) {
  if (s->phA.groups.empty() || s->gp.big_g < 0) return P_<uint8_t>(s->d_gath) + 576 * LSG_MAX_DEVICES;
  return P_<uint8_t>(s->d_Fb) + 576 * (size_t)s->gp.big_g;
}

// The package group's partial as it may leave the slot (lsg_jobs_partial*), on the main stream:
// a lone unscaled set's f is raised to a fresh nonzero 64-bit randomizer (two
// one-set shards holding sig_a + D and sig_b - D must not pass a product check together).
// xs: launch the power there instead of on the slot's stream (the partial is complete)
int export_partial_dev(Slot* s, const uint8_t** src, hipStream_t xs = nullptr) {
  *src = pkg_partial_dev(s);
  if (!s->gp.lone_unscaled) return LSG_OK;
  uint64_t r = 0;
  if (s->seed) {  // tests: reproducible
    uint64_t sd = s->seed ^ 0x5851f42d4c957f2dull;
    do r = splitmix64(sd);
    while (r == 0);
  } else {
    do {
      if (!os_random(&r, 8)) {
        set_err(s->d->c, "no entropy for the exported partial's randomizer (getrandom failed)");
        return LSG_ERR_ENTROPY;
      }
    } while (r == 0);
  }
  LSG_RC(ensure(s, s->d_xport, 576));
  s->cur = 0;
  if (xs) {
    const hipError_t e = lsgk::fp12_pow_u64(xs, *src, r, P_<uint8_t>(s->d_xport));
    if (e != hipSuccess) return fail(s, "k_fp12_pow", e);
  } else {
    KL(s, "k_fp12_pow", lsgk::fp12_pow_u64(S_(s), *src, r, P_<uint8_t>(s->d_xport)));
  }
  *src = P_<uint8_t>(s->d_xport);
  return LSG_OK;
}

// node check on this slot (device 0 of the ticket): product of the n gathered partials in
// d_gath, one final exponentiation -> h_nodeV (ev_node)
int pkg_node_check(Slot* s, int n) {
  s->cur = 0;
  const uint32_t* nf = P_<uint32_t>(s->d_nodeF);
  KL(s, "k_blobs_to_fp12", lsgk::blobs_to_fp12(S_(s), n, P_<uint8_t>(s->d_gath), P_<uint32_t>(s->d_nodeF)));
  LSG_RC(run_seg(s, 2, "fp12_product", s->phA_node, nf, P_<uint32_t>(s->d_nodeF) + W_F12 * (size_t)n));
  uint8_t* blob = P_<uint8_t>(s->d_gath) + 576 * (size_t)(LSG_MAX_DEVICES + 1);
  KL(s, "k_fp12_to_canon", lsgk::fp12_to_canon(S_(s), 1, P_<uint32_t>(s->d_nodeF) + W_F12 * (size_t)n, blob));
  KL(s, "slp_final_exp", lsg_slp_final_exp(S_(s), 1, blob, P_<int32_t>(s->d_nodeV)));
  LSG_HIP(s, hipMemcpyAsync(s->h_nodeV.p, s->d_nodeV.p, 4, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipEventRecord(s->ev_node, s->st[0]));
  return LSG_OK;
}

// Part 2 of phase A: every group's final exponentiation and the status readback (ev_done).
// skip_big (a multi-device ticket): the package group's final exponentiation is left out --
// the node check over all devices' partials decides it (one final
// exponentiation per node), and it runs only when that check fails (pkg_resolve).
int pkg_part2(Slot* s, bool skip_big = false) {
  const size_t ng = s->phA.groups.size();
  s->big_fe_pending = skip_big && !s->gp.chunk_mode && s->gp.big_g >= 0;
  if (s->big_fe_pending) {
    LSG_RC(launch_fe_range(s, 0, (size_t)s->gp.big_g));
    LSG_RC(launch_fe_range(s, (size_t)s->gp.big_g + 1, ng));
  } else {
    LSG_RC(launch_fe(s, ng));
  }
  return launch_readback(s, true);
}

// One fallback phase (worker.ts:74-96) over `groups` (scaled signature sums, own Miller items
// into fall2), synchronous; verdicts into v.
// The context mutex is released while a fallback phase runs on the device (the ticket's slots
// stay claimed, so no other caller touches them): other threads keep submitting and resolving.
typedef std::unique_lock<std::mutex> CtxLock;

// One fallback phase (worker.ts:74-96) over `groups` (scaled signature sums), synchronous;
// verdicts into v.  given: per group, its items among phase A's resident Miller items (the
// package group's chunk-aligned items: no new Miller accumulation); else the phase plans and
// accumulates its own items (into fall2).
int run_fallback_phase(Slot* s, CtxLock* lk, const std::vector<Grp>& groups,
                       const std::vector<std::pair<int32_t, int32_t>>* given, std::vector<int32_t>& v) {
  v.assign(groups.size(), 0);
  if (groups.empty()) return LSG_OK;
  const uint64_t tf0 = trace_host() ? now_ns() : 0;
  // Signature sums: a group whose sets were all in a phase-A bucket-MSM group (rs_raw) and that
  // is large enough sums them by its own bucket MSM (no per-set scaling): its bucket pass reads
  // the resident affine signatures (LSG_MSM_FOLD=0: their unscaled copies in d_rs, which only
  // such sets have); the others sum [r_i] sig_i (d_rs2, scaled below).  MSM groups go first
  // (plan_phase); `order` maps the phase's group k to the caller's.
  std::vector<size_t> order;
  std::vector<uint8_t> gm(groups.size(), 0);
  for (size_t g = 0; g < groups.size(); g++) {
    bool ok = groups[g].len >= std::max(s->sw.msm_min_group, (size_t)2) && s->rs_raw.size() == s->n_sets;
    for (size_t i = groups[g].first; ok && i < groups[g].first + groups[g].len; i++) ok = s->rs_raw[i] != 0;
    gm[g] = ok;
    if (ok) order.push_back(g);
  }
  const size_t n_msm = order.size();
  for (size_t g = 0; g < groups.size(); g++)
    if (!gm[g]) order.push_back(g);
  // size this phase's buffers BEFORE any pointer into them is taken or any launch queued:
  // a phase with more groups than phase A had grows d_fall2 (and the group buffers), and a
  // pointer saved earlier would name the freed allocation
  LSG_RC(size_state(s, s->n_sets, s->n_pks, groups.size(), n_msm, 2));
  s->cur = 0;  // the phase's kernel timers follow phase A's (lsg_last_kernel_times: the whole ticket)
  s->plan.clear();
  PhasePlan Ph;
  for (size_t k = 0; k < order.size(); k++) {
    Ph.groups.push_back(groups[order[k]]);
    Ph.groups.back().msm = gm[order[k]] != 0;
  }
  // groups of one set each (the per-job phase of single-set jobs): one-set Miller items in
  // the list form instead of four-wave fused items holding one pair
  size_t singles = 0;
  for (auto& g : groups) singles += g.len == 1 ? 1 : 0;
  const int K = !given && 2 * singles >= groups.size() ? 1 : s->K;
  if (given) {
    Ph.reuse_items = true;
    for (size_t k = 0; k < order.size(); k++) Ph.given.push_back((*given)[order[k]]);
    Ph.n_items = s->phA.n_items;
    Ph.term_base = s->phA.n_items + s->phA.groups.size();  // after phase A's own terms
  }
  plan_phase(s->plan, s->rnd, K, s->sw, Ph);
  LSG_RC(upload_plan(s));
  // [r_i] sig_i into d_rs2 for the sets no earlier fallback phase of this package scaled
  if (s->rs2_scaled.size() != s->n_sets) s->rs2_scaled.assign(s->n_sets, 0);
  std::vector<uint8_t> mode(s->n_sets, 0);
  bool any = false;
  for (size_t g = 0; g < groups.size(); g++) {
    if (gm[g]) continue;  // (its MSM scales by buckets)
    for (size_t i = groups[g].first; i < groups[g].first + groups[g].len; i++)
      if (!s->rs2_scaled[i]) {
        mode[i] = s->rs2_scaled[i] = 1;
        any = true;
      }
  }
  // the side stream needs the plan: order it after the upload on the main stream
  LSG_HIP(s, hipEventRecord(s->ev_in, s->st[0]));
  LSG_HIP(s, hipStreamWaitEvent(s->st[1], s->ev_in, 0));
  if (any) {
    s->cur = 1;
    const int n = (int)s->n_sets;
    LSG_RC(ensure_host(s, s->h_mode, (size_t)n));
    memcpy(s->h_mode.p, mode.data(), (size_t)n);
    LSG_HIP(s, hipMemcpyAsync(s->d_mode.p, s->h_mode.p, (size_t)n, hipMemcpyHostToDevice, s->st[1]));
    size_t n_scaled = 0;
    for (uint8_t m : mode) n_scaled += m;
    if (slp_items_max() > 0 && n_scaled <= 8192)  // one program per scaled set (the others exit at once)
      KL(s, "k_slp_g2_scale", lsg_slp_g2_scale(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                               P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), P_<uint64_t>(s->d_rnd),
                                               P_<uint8_t>(s->d_mode), P_<uint32_t>(s->d_rs2)));
    else
      KL(s, "k_sig_scale", lsgk::sig_scale_only(S_(s), n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                                P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), P_<uint64_t>(s->d_rnd),
                                                P_<uint8_t>(s->d_mode), P_<uint32_t>(s->d_rs2)));
  }
  s->cur = 0;
  uint32_t* fall = given ? P_<uint32_t>(s->d_fall) : P_<uint32_t>(s->d_fall2);
  if (!given) LSG_RC(launch_accum(s, Ph.n_items, Ph.item_off, fall, Ph.single_items));
  LSG_RC(launch_phase(s, Ph, P_<uint32_t>(s->d_rs2), fall, false, P_<uint32_t>(s->d_rs)));
  LSG_RC(launch_fe(s, groups.size()));
  LSG_RC(launch_readback(s, false));
  const uint64_t tf1 = trace_host() ? now_ns() : 0;
  const int dev = s->d->device;
  if (lk) lk->unlock();
  hipError_t e = event_wait(s->ev_done);
  if (lk) {
    lk->lock();
    (void)hipSetDevice(dev);
  }
  if (e != hipSuccess) return fail(s, "hipEventSynchronize", e);
  if (trace_host())
    fprintf(stderr, "lsg host: fallback groups %zu (msm %zu) given %d | plan+launch %.3f ms, device+lock %.3f ms\n",
            groups.size(), n_msm, given ? 1 : 0, (tf1 - tf0) * 1e-6, (now_ns() - tf1) * 1e-6);
  s->stats.n_final_exps += (uint32_t)groups.size();
  for (size_t k = 0; k < order.size(); k++) v[order[k]] = H_<int32_t>(s->h_verdict)[k];
  return LSG_OK;
}

// the deferred final exponentiation of the package group (pkg_part2 skip_big), synchronous
int run_big_fe(Slot* s, CtxLock* lk) {
  s->cur = 0;
  LSG_RC(launch_fe_range(s, (size_t)s->gp.big_g, (size_t)s->gp.big_g + 1));
  LSG_HIP(s, hipEventRecord(s->ev_done, s->st[0]));
  const int dev = s->d->device;
  if (lk) lk->unlock();
  hipError_t e = event_wait(s->ev_done);
  if (lk) {
    lk->lock();
    (void)hipSetDevice(dev);
  }
  if (e != hipSuccess) return fail(s, "hipEventSynchronize", e);
  s->big_fe_pending = false;
  return LSG_OK;
}

// The first bad key of this device's share in caller order (lsgp::first_key_error; 0: none)
// and the caller index of its job.
int32_t first_pk_error(Slot* s, size_t* job_id) {
  size_t k = 0;
  const int32_t e = first_key_error(s->shape, H_<int32_t>(s->h_pkerr), 0, s->shape.jobs.size(), &k);
  if (e) *job_id = s->shape.job_ids[k];
  return e;
}

// The reference's verdict rules for this device's share of the package (worker.ts:30-106),
// after ev_done: lsgp::resolve_package over the phase-A verdicts, its group checks run here
// as fallback phases.  node_valid: 1 = the node-wide check of all devices' partials passed,
// 0 = it failed (this device's own package check localises), -1 = no node check (single
// device), 2 = this ticket's own node check (lsg_init_devices: the library gathered every
// device's partial itself) passed, and it decides a package group whose final exponentiation
// was deferred.  Otherwise the node-wide verdict is advisory (resolve_package).
// pkfail: the package-wide deserializeSet failure (first_pk_error over every device of the
// ticket, in caller order) -- a bad key on any device rejects every job of the package
int pkg_resolve(Slot* s, CtxLock* lk, int node_valid, int32_t pkfail) {
  const SetStatus ss = read_status(s);
  const PhasePlan& A = s->phA;
  std::vector<int32_t> vA(H_<int32_t>(s->h_verdict), H_<int32_t>(s->h_verdict) + A.groups.size());
  s->stats.n_final_exps += (uint32_t)(A.groups.size() - (s->big_fe_pending ? 1 : 0));
  if (s->big_fe_pending && !pkfail) {
    if (node_valid == 2) {
      vA[(size_t)s->gp.big_g] = 1;
    } else {  // the node check failed: this device's own check localises
      LSG_RC(run_big_fe(s, lk));
      vA[(size_t)s->gp.big_g] = H_<int32_t>(s->h_verdict)[s->gp.big_g];
      s->stats.n_final_exps++;
    }
  }
  const CheckFn check = [&](const std::vector<Grp>& groups, const std::vector<ItemRange>* given, std::vector<int32_t>& v) {
    return run_fallback_phase(s, lk, groups, given, v);
  };
  return resolve_package(s->shape, s->gp, ss, vA, pkfail, A, s->sw, check,
                         PkgVerdicts{s->results, s->stats, s->sub_stats, s->sub_pkfail});
}

}  // namespace

// ---------------------------------------------------------------------------- tickets
namespace {

uint64_t make_ticket(lsg_ctx* c, int kind, int index, uint64_t* serial) {
  *serial = c->next_serial++;
  return (*serial << 16) | ((uint64_t)kind << 8) | (uint64_t)index;
}

// package index of a jobs ticket (slot `index` on every device), or -1
int ticket_pkg(lsg_ctx* c, uint64_t t) {
  const int k = (int)((t >> 8) & 255), i = (int)(t & 255);
  if (k != SLOT_JOBS || i >= LSG_SLOTS) return -1;
  const Slot& s = c->dev[0]->slots[i];
  if (s.kind != SLOT_JOBS || s.serial != (t >> 16)) return -1;
  return i;
}
Slot* ticket_final(lsg_ctx* c, uint64_t t) {
  const int k = (int)((t >> 8) & 255), i = (int)(t & 255);
  if (k != SLOT_FINAL || i >= LSG_FINALS) return nullptr;
  Slot* s = &c->dev[0]->finals[i];
  if (s->kind != SLOT_FINAL || s->serial != (t >> 16)) return nullptr;
  return s;
}

// The slot's launch is over for the message cache: its pinned rows are unpinned and the rows it
// wrote become visible (ok: the host has observed the launch's completion) or free (a failed
// submit, after sync_slot).  Idempotent: the first of wait and poll to observe it settles.
void mc_settle(Slot* s, bool ok) {
  if (!s->mc_on) return;
  MsgCache& mc = s->d->mc;
  mc.unpin(s->mc_epoch, s->mc_pins.data(), s->mc_pins.size());
  if (ok)
    mc.publish(s->mc_epoch, s->mc_pend.data(), s->mc_pend.size());
  else
    mc.drop(s->mc_epoch, s->mc_pend.data(), s->mc_pend.size());
  s->mc_pins.clear();
  s->mc_pend.clear();
  s->mc_on = false;
}

void sync_slot(Slot* s) {
  for (int k = 0; k < 2; k++)
    if (s->st[k]) (void)hipStreamSynchronize(s->st[k]);
}

bool force_exchange() { return lsg_ab_long("LSG_FORCE_EXCHANGE", 0) != 0; }

// all-gather of the devices' partials into device 0's d_gath, then the node check there
int pkg_exchange(lsg_ctx* c, int p) {
  const int n = c->n_dev;
  Slot* s0 = &c->dev[0]->slots[p];
  if (c->rccl) {
    // one collective over xGMI: every device contributes 576 bytes
    ncclResult_t r = ncclGroupStart();
    for (int d = 0; d < n && r == ncclSuccess; d++) {
      Slot* s = &c->dev[d]->slots[p];
      (void)hipSetDevice(c->dev[d]->device);
      r = ncclAllGather(pkg_partial_dev(s), s->d_gath.p, 576, ncclUint8, c->comm[d], s->st[0]);
    }
    ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    (void)hipSetDevice(c->dev[0]->device);
    if (r != ncclSuccess) {
      set_err(c, std::string("ncclAllGather: ") + ncclGetErrorString(r));
      return LSG_ERR_DEVICE;
    }
  } else {
    // duplicate device list (tests): device-to-device copies on device 0's main stream
    (void)hipSetDevice(c->dev[0]->device);
    for (int d = 0; d < n; d++) {
      Slot* s = &c->dev[d]->slots[p];
      LSG_HIP(s0, hipStreamWaitEvent(s0->st[0], s->ev_part, 0));
      uint8_t* dst = P_<uint8_t>(s0->d_gath) + 576 * (size_t)d;
      if (c->dev[d]->device == c->dev[0]->device)
        LSG_HIP(s0, hipMemcpyAsync(dst, pkg_partial_dev(s), 576, hipMemcpyDeviceToDevice, s0->st[0]));
      else
        LSG_HIP(s0, hipMemcpyPeerAsync(dst, c->dev[0]->device, pkg_partial_dev(s), c->dev[d]->device, 576, s0->st[0]));
    }
  }
  return pkg_node_check(s0, n);
}

// Each device's share of a package (pkg_part1 .. pkg_part2), staged with the context lock
// released: device 0 on the calling thread, every other device on a thread of its own, so that
// a context over N GPUs spends one device's staging time per package instead of N (VERDICT r5
// item 3), and host threads submitting packages to different slots stage them side by side.
// Errors go to *err (t_err_sink), not to c->err.
int stage_pkg(lsg_ctx* c, int p, const lsg_job* jobs, size_t n_jobs, uint64_t seed, bool lone_ok, bool exch,
              std::string* err, const uint8_t* dev_msgs = nullptr, const uint32_t* set_group = nullptr,
              size_t n_groups = 0, const uint64_t* rnd_in = nullptr, bool msg_cache = true) {
  const int n = c->n_dev;
  std::vector<std::vector<size_t>> ids(n);
  {
    std::vector<uint32_t> sizes(n_jobs);
    std::vector<int32_t> owner(n_jobs);
    for (size_t j = 0; j < n_jobs; j++) sizes[j] = jobs[j].n_sets;
    assign_jobs(sizes.data(), n_jobs, n, owner.data());
    for (size_t j = 0; j < n_jobs; j++) ids[(size_t)owner[j]].push_back(j);
  }
  std::vector<int> rcs(n, LSG_OK);
  std::vector<std::string> errs(n);
  auto part1 = [&](int d) {
    t_err_sink = &errs[d];
    (void)hipSetDevice(c->dev[d]->device);
    // distinct seeds per device for tests; 0 stays 0 (OS CSPRNG on every device)
    const uint64_t sd = seed ? seed + 0x9e3779b97f4a7c15ull * (uint64_t)d : 0;
    rcs[d] = pkg_part1(&c->dev[d]->slots[p], jobs, ids[d], sd, (d == 0 && exch) ? n : 0, nullptr, lone_ok && !exch,
                       n == 1 ? dev_msgs : nullptr, n == 1 ? set_group : nullptr, n_groups, n == 1 ? rnd_in : nullptr,
                       msg_cache);
    t_err_sink = nullptr;
  };
  auto part2 = [&](int d) {
    t_err_sink = &errs[d];
    (void)hipSetDevice(c->dev[d]->device);
    rcs[d] = pkg_part2(&c->dev[d]->slots[p], exch);
    t_err_sink = nullptr;
  };
  // first error in device order
  auto first_rc = [&]() {
    for (int d = 0; d < n; d++)
      if (rcs[d]) {
        *err = errs[d];
        return rcs[d];
      }
    return (int)LSG_OK;
  };
  std::shared_lock<std::shared_mutex> tab(c->tab_mu);  // (the sets may name table rows)
  int rc = LSG_OK;
  // A/B build: LSG_STAGE_PAR=0 stages the devices one after another (round 5), 1 runs part 1
  // on threads and part 2 serially, 2 (shipped) both on threads
  const long par = n == 1 ? 0 : lsg_ab_long("LSG_STAGE_PAR", 2);
  if (par == 0) {
    for (int d = 0; d < n && !rc; d++) {
      part1(d);
      rc = first_rc();
    }
    if (!rc && exch) {
      std::lock_guard<std::mutex> x(c->xmu);
      t_err_sink = err;
      rc = pkg_exchange(c, p);
      t_err_sink = nullptr;
    }
    for (int d = 0; d < n && !rc; d++) {
      part2(d);
      rc = first_rc();
    }
    return rc;
  }
  // devices 1..n-1 on threads of their own: part 1, then (after the exchange, which needs every
  // device's partial) part 2
  std::mutex m;
  std::condition_variable cv;
  int n_part1 = 1;  // devices done with part 1 (device 0 counted when it is)
  int phase2 = 0;   // 1: run part 2, -1: stop (an error before the exchange or in it)
  std::vector<std::thread> th;
  for (int d = 1; d < n; d++)
    th.emplace_back([&, d] {
      part1(d);
      std::unique_lock<std::mutex> l(m);
      n_part1++;
      cv.notify_all();
      cv.wait(l, [&] { return phase2 != 0; });
      const bool go = phase2 > 0 && par >= 2;
      l.unlock();
      if (go) part2(d);
    });
  part1(0);
  {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return n_part1 == n; });
  }
  rc = first_rc();
  if (!rc && exch) {
    std::lock_guard<std::mutex> x(c->xmu);  // one exchange at a time over the communicators
    t_err_sink = err;
    rc = pkg_exchange(c, p);
    t_err_sink = nullptr;
  }
  {
    std::lock_guard<std::mutex> l(m);
    phase2 = rc ? -1 : 1;
  }
  cv.notify_all();
  if (!rc) part2(0);
  for (int d = 1; d < n && !rc && par < 2; d++) {
    part2(d);
    rc = first_rc();
  }
  for (auto& t : th) t.join();
  if (!rc) rc = first_rc();
  return rc;
}

// A package: its slot is reserved on every device under the context lock (`lk`, held on entry
// and on return), staged with the lock released (stage_pkg), and its ticket committed under the
// lock again.  A reserved slot is SLOT_STAGING: no other call takes, reserves or waits on it.
int submit_pkg(lsg_ctx* c, CtxLock& lk, const lsg_job* jobs, size_t n_jobs, uint64_t seed, lsg_ticket* ticket,
               bool lone_ok = true, const uint8_t* dev_msgs = nullptr, const uint32_t* set_group = nullptr,
               size_t n_groups = 0, const uint64_t* rnd_in = nullptr, bool msg_cache = true) {
  int p = -1;
  for (int i = 0; i < LSG_SLOTS && p < 0; i++)
    if (c->dev[0]->slots[i].kind == SLOT_FREE) p = i;
  if (p < 0) {
    c->err = "all pipeline slots are busy (wait on an outstanding ticket first)";
    return LSG_ERR_BUSY;
  }
  const int n = c->n_dev;
  const bool exch = n > 1 || force_exchange();
  bool prio = false;
  for (size_t j = 0; j < n_jobs; j++) prio = prio || (jobs[j].flags & LSG_JOB_PRIORITY) != 0;
  for (int d = 0; d < n; d++) {
    (void)hipSetDevice(c->dev[d]->device);
    LSG_RC(slot_ready(c->dev[d], &c->dev[d]->slots[p], p));
    LSG_RC(slot_streams(&c->dev[d]->slots[p], prio));
  }
  for (int d = 0; d < n; d++) c->dev[d]->slots[p].kind = SLOT_STAGING;
  c->staging++;
  lk.unlock();
  std::string err;
  const int rc = stage_pkg(c, p, jobs, n_jobs, seed, lone_ok, exch, &err, dev_msgs, set_group, n_groups, rnd_in, msg_cache);
  lk.lock();
  (void)hipSetDevice(c->dev[0]->device);
  c->staging--;
  c->cv.notify_all();
  if (rc) {
    for (int d = 0; d < n; d++) {
      sync_slot(&c->dev[d]->slots[p]);
      mc_settle(&c->dev[d]->slots[p], false);
      c->dev[d]->slots[p].kind = SLOT_FREE;
    }
    c->err = err;
    return rc;
  }
  uint64_t serial;
  *ticket = make_ticket(c, SLOT_JOBS, p, &serial);
  for (int d = 0; d < n; d++) {
    Slot* s = &c->dev[d]->slots[p];
    s->kind = SLOT_JOBS;
    s->serial = serial;
  }
  c->dev[0]->slots[p].n_jobs = n_jobs;
  c->dev[0]->slots[p].stats.submit_us = (uint32_t)((now_ns() - c->dev[0]->slots[p].stats.start_ns) / 1000);
  return LSG_OK;
}

// The aggregates of a resolved grouped package (single device): per group the compressed sum of
// the signatures of the sets whose job resolved to LSG_VALID, and how many they were.  When
// every grouped set is included (the common case) the sums launched at submit stand; otherwise
// they are planned again over the included sets and launched once more on the slot's main
// stream (the per-set values are resident, as for the fallback phases), synchronously.
int finish_sig_groups(Slot* s, CtxLock* lk, uint8_t* agg96, uint32_t* agg_n) {
  const size_t ng = s->grp_n;
  std::vector<uint32_t> cnt(ng, 0);
  size_t left_out = 0, included = 0;
  for (size_t k = 0; k < s->shape.jobs.size(); k++) {
    const JobRec& J = s->shape.jobs[k];
    const bool valid = s->results[k].status == LSG_VALID;
    for (size_t i = J.first; i < J.first + J.count; i++) {
      if (s->set_grp[i] == LSG_NO_GROUP) continue;
      if (valid) {
        cnt[s->set_grp[i]]++;
        included++;
      } else {
        left_out++;
      }
    }
  }
  if (left_out && included) {
    const std::vector<uint8_t> mask = included_sets(s->shape, s->results.data());
    s->cur = 0;
    LSG_RC(run_sig_groups(s, mask.data()));
    LSG_HIP(s, hipEventRecord(s->ev_done, s->st[0]));
    const int dev = s->d->device;
    if (lk) lk->unlock();
    hipError_t e = event_wait(s->ev_done);
    if (lk) {
      lk->lock();
      (void)hipSetDevice(dev);
    }
    if (e != hipSuccess) return fail(s, "hipEventSynchronize", e);
  }
  for (size_t g = 0; g < ng; g++) {
    agg_n[g] = cnt[g];
    if (cnt[g])
      memcpy(agg96 + 96 * g, H_<uint8_t>(s->h_gagg) + 96 * g, 96);
    else
      memset(agg96 + 96 * g, 0, 96);
  }
  return LSG_OK;
}

// resolve a package: node_valid as pkg_resolve (-2: the ticket's own node check); agg96 /
// agg_n: the aggregates of a grouped package (null: dropped)
int wait_pkg(lsg_ctx* c, CtxLock* lk, int p, int node_valid, lsg_job_result* results, lsg_stats* stats,
             uint8_t* agg96 = nullptr, uint32_t* agg_n = nullptr) {
  const int n = c->n_dev;
  int rc = LSG_OK;
  for (int d = 0; d < n && !rc; d++) {
    Slot* s = &c->dev[d]->slots[p];
    (void)hipSetDevice(c->dev[d]->device);
    if (event_wait(s->ev_done) != hipSuccess) rc = fail(s, "hipEventSynchronize", hipGetLastError());
  }
  for (int d = 0; d < n; d++) mc_settle(&c->dev[d]->slots[p], rc == LSG_OK);
  Slot* s0 = &c->dev[0]->slots[p];
  // the ticket's own node check (lsg_init_devices) decides the package groups: 2 = passed
  if (!rc && node_valid == -2) node_valid = s0->has_node ? (H_<int32_t>(s0->h_nodeV)[0] ? 2 : 0) : -1;
  lsg_stats total;
  memset(&total, 0, sizeof(total));
  total.start_ns = s0->stats.start_ns;
  total.submit_us = s0->stats.submit_us;
  int32_t pkfail = 0;  // package-wide: the first bad key in caller job order over all devices
  size_t pkfail_job = SIZE_MAX;
  for (int d = 0; d < n && !rc; d++) {
    size_t j = SIZE_MAX;
    const int32_t e = first_pk_error(&c->dev[d]->slots[p], &j);
    if (e && j < pkfail_job) {
      pkfail = e;
      pkfail_job = j;
    }
  }
  for (int d = 0; d < n && !rc; d++) {
    Slot* s = &c->dev[d]->slots[p];
    (void)hipSetDevice(c->dev[d]->device);
    rc = pkg_resolve(s, lk, node_valid, pkfail);
    if (rc) break;
    for (size_t k = 0; k < s->shape.jobs.size(); k++) results[s->shape.job_ids[k]] = s->results[k];
    total.batch_retries += s->stats.batch_retries;
    total.batch_sigs_success += s->stats.batch_sigs_success;
    total.n_final_exps += s->stats.n_final_exps;
  }
  if (!rc && agg96 && agg_n && s0->grp_n) rc = finish_sig_groups(s0, lk, agg96, agg_n);
  if (s0->has_node) total.n_final_exps += 1;
  total.key_error = pkfail;
  total.key_error_job = pkfail ? (uint32_t)pkfail_job : 0;
  total.end_ns = now_ns();
  if (stats) *stats = total;
  for (int d = 0; d < n; d++) {
    Slot* s = &c->dev[d]->slots[p];
    if (rc) sync_slot(s);
    s->kind = SLOT_FREE;
    keep_times(s);
  }
  (void)hipSetDevice(c->dev[0]->device);
  return rc;
}

// ---- coalesced launches (lsg_set_coalesce)
// bytes behind a set's pks: key slots, table indices, or a committee id + its bitfield
size_t set_key_bytes(const lsg_set& t) {
  if (!t.pks) return 0;
  if (t.pk_len == LSG_PK_BITS) return 4 + (((size_t)t.n_pks + 7) >> 3);
  if (t.pk_len == LSG_PK_BITS_MULTI) return 4 + 4 * (size_t)multi_k(t) + (((size_t)t.n_pks + 7) >> 3);  // (k checked on entry)
  return (size_t)t.n_pks * (t.pk_len == LSG_PK_INDEX ? 4 : t.pk_len);
}
PendingPkg copy_pkg(const lsg_job* jobs, size_t n_jobs, uint64_t seed) {
  PendingPkg pk;
  pk.seed = seed;
  size_t ns = 0, nb = 0;
  for (size_t j = 0; j < n_jobs; j++)
    for (uint32_t q = 0; q < jobs[j].n_sets; q++) {
      const lsg_set& t = jobs[j].sets[q];
      ns++;
      nb += set_key_bytes(t) + (t.msg ? msg_bytes(t.msg_len) : 0) +
            (t.sig ? t.sig_len : 0);
    }
  pk.n_sets = ns;
  pk.sets.resize(ns);
  pk.data.resize(std::max(nb, (size_t)1));
  pk.jobs.assign(jobs, jobs + n_jobs);
  size_t si = 0, off = 0;
  auto put = [&](const uint8_t* src, size_t len) -> const uint8_t* {
    if (!src) return nullptr;
    uint8_t* d = pk.data.data() + off;
    if (len) memcpy(d, src, len);
    off += len;
    return d;
  };
  for (size_t j = 0; j < n_jobs; j++) {
    pk.jobs[j].sets = pk.sets.data() + si;
    for (uint32_t q = 0; q < jobs[j].n_sets; q++, si++) {
      lsg_set t = jobs[j].sets[q];
      t.pks = put(t.pks, set_key_bytes(t));
      t.msg = put(t.msg, t.msg ? msg_bytes(t.msg_len) : 0);
      t.sig = put(t.sig, t.sig ? t.sig_len : 0);
      pk.sets[si] = t;
    }
  }
  return pk;
}

// launches still executing on the device (their completion event not reached): a launch
// whose work is done no longer holds packages back, whether or not its tickets were waited on
int launches_in_flight(lsg_ctx* c) {
  int n = 0;
  for (int i = 0; i < LSG_SLOTS; i++) {
    const Slot& s = c->dev[0]->slots[i];
    n += s.kind == SLOT_JOBS && hipEventQuery(s.ev_done) == hipErrorNotReady ? 1 : 0;
  }
  return n;
}

// the pending packages as one launch: one slot, each package a sub-package with its own
// chunks, deserialisation rule and counters (context lock held)
int flush_pending(lsg_ctx* c) {
  if (c->pending.empty()) return LSG_OK;
  int p = -1;
  for (int i = 0; i < LSG_SLOTS && p < 0; i++)
    if (c->dev[0]->slots[i].kind == SLOT_FREE) p = i;
  if (p < 0) {
    c->err = "all pipeline slots are busy (wait on an outstanding ticket first)";
    return LSG_ERR_BUSY;
  }
  Slot* s = &c->dev[0]->slots[p];
  LSG_RC(slot_ready(c->dev[0], s, p));
  LSG_RC(slot_streams(s, false));
  std::vector<lsg_job> all;
  std::vector<size_t> subs{0};
  uint64_t seed = c->pending[0].seed;
  for (auto& pk : c->pending) {
    all.insert(all.end(), pk.jobs.begin(), pk.jobs.end());
    subs.push_back(all.size());
    if (!pk.seed) seed = 0;  // any package asking for OS randomness gets it for all
  }
  std::vector<size_t> ids(all.size());
  for (size_t j = 0; j < ids.size(); j++) ids[j] = j;
  int rc = pkg_part1(s, all.data(), ids, seed, 0, &subs);
  if (!rc) rc = pkg_part2(s);
  if (rc) {
    sync_slot(s);
    mc_settle(s, false);
    // every held package's wait (or poll) reports this failure -- its code and message --
    // instead of an unknown ticket; the entry goes when its ticket is waited on
    for (auto& pk : c->pending) {
      MergeTicket& m = c->merged[pk.serial];
      m.slot = -1;
      m.rc = rc;
      m.err = c->err;
    }
    c->pending.clear();
    c->pending_sets = 0;
    return rc;
  }
  uint64_t serial;
  (void)make_ticket(c, SLOT_JOBS, p, &serial);
  s->kind = SLOT_JOBS;
  s->serial = serial;
  s->n_jobs = all.size();
  s->sub_serial.clear();
  for (size_t k = 0; k < c->pending.size(); k++) {
    s->sub_serial.push_back(c->pending[k].serial);
    c->merged[c->pending[k].serial] = MergeTicket{p, (int)k};
  }
  s->stats.submit_us = (uint32_t)((now_ns() - s->stats.start_ns) / 1000);
  c->pending.clear();
  c->pending_sets = 0;
  return LSG_OK;
}

// launch what is pending when the device has room (after a wait freed a slot)
void maybe_flush(lsg_ctx* c) {
  if (!c->pending.empty() && launches_in_flight(c) < c->co_inflight) (void)flush_pending(c);
}

int submit_merged(lsg_ctx* c, const lsg_job* jobs, size_t n_jobs, uint64_t seed, size_t n_sets, lsg_ticket* ticket) {
  if (c->pending_sets + n_sets > c->co_max_pending) LSG_RC(flush_pending(c));
  PendingPkg pk = copy_pkg(jobs, n_jobs, seed);
  uint64_t serial;
  *ticket = make_ticket(c, SLOT_MERGE, 0, &serial);
  pk.serial = serial;
  c->merged[serial] = MergeTicket{};
  c->pending.push_back(std::move(pk));
  c->pending_sets += n_sets;
  if (launches_in_flight(c) < c->co_inflight) {
    const int rc = flush_pending(c);
    if (rc && rc != LSG_ERR_BUSY) {  // (busy: it stays pending, a later wait launches it)
      c->merged.erase(serial);       // this submission fails; the others' waits report rc
      return rc;
    }
  }
  return LSG_OK;
}

int wait_merged(lsg_ctx* c, lsg_ticket t, lsg_job_result* results, lsg_stats* stats) {
  const uint64_t serial = t >> 16;
  int p, k;
  hipEvent_t ev;
  for (int spin = 0;; spin++) {
    std::unique_lock<std::mutex> lk(c->mu);
    LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
    auto it = c->merged.find(serial);
    if (it == c->merged.end()) return LSG_ERR_INVALID_ARG;
    if (it->second.slot >= 0 || it->second.rc) break;  // launched (or its launch failed)
    // still held: it goes out with whatever else is pending once fewer than co_inflight launches
    // execute -- packages submitted meanwhile join it (a waiter forcing the flush at once left
    // two packages per launch on the gossip bench) -- or at once if the device is idle
    if (launches_in_flight(c) >= c->co_inflight) {
      lk.unlock();
      std::this_thread::sleep_for(std::chrono::microseconds(spin < 20 ? 50 : 200));
      continue;
    }
    const int frc = flush_pending(c);
    it = c->merged.find(serial);
    if (it == c->merged.end()) return LSG_ERR_INVALID_ARG;
    // still held (every slot busy: LSG_ERR_BUSY, c->err says so): the ticket stays live and a
    // later wait -- after the caller has waited on another ticket -- launches it
    if (frc && it->second.slot < 0 && !it->second.rc) return frc;
    break;
  }
  {
    std::lock_guard<std::mutex> lk(c->mu);
    LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
    auto it = c->merged.find(serial);
    if (it == c->merged.end()) return LSG_ERR_INVALID_ARG;
    if (it->second.rc) {  // its coalesced launch failed
      const int frc = it->second.rc;
      c->err = it->second.err;
      c->merged.erase(it);
      return frc;
    }
    if (it->second.slot < 0) return LSG_ERR_INVALID_ARG;
    p = it->second.slot;
    k = it->second.sub;
    ev = c->dev[0]->slots[p].ev_done;
  }
  const hipError_t wr = event_wait(ev);
  CtxLock lk(c->mu);
  if (wr != hipSuccess) return fail_c(c, "hipEventSynchronize", wr);
  LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
  Slot* s = &c->dev[0]->slots[p];
  c->cv.wait(lk, [&] { return !s->resolving; });
  mc_settle(s, true);
  if (!s->resolved) {  // the first waiter resolves every sub-package (fallback phases included)
    s->resolving = true;
    s->resolve_rc = pkg_resolve(s, &lk, -1, 0);
    s->resolved = true;
    s->resolving = false;
    c->cv.notify_all();
  }
  const int rc = s->resolve_rc;
  for (size_t j = s->shape.sub_first[k]; j < s->shape.sub_first[k + 1]; j++) results[j - s->shape.sub_first[k]] = s->results[j];
  if (stats) {
    *stats = s->sub_stats[k];
    stats->start_ns = s->stats.start_ns;
    stats->submit_us = s->stats.submit_us;
    stats->n_final_exps = s->stats.n_final_exps;  // (the whole coalesced launch)
    stats->end_ns = now_ns();
  }
  c->merged.erase(serial);
  s->sub_done[k] = 1;
  bool all = true;
  for (uint8_t d : s->sub_done) all = all && d;
  if (all) {
    if (rc) sync_slot(s);
    s->kind = SLOT_FREE;
    s->shape.n_sub = 0;
    keep_times(s);
    maybe_flush(c);
  }
  return rc;
}

#define LSG_ENTER(c)                         \
  std::lock_guard<std::mutex> _lk((c)->mu); \
  LSG_HIPC((c), hipSetDevice((c)->dev[0]->device))

// Block until a ticket's device work is done WITHOUT holding the context mutex, so a waiter
// (e.g. an N-API worker thread) never stalls submissions from another thread.  The ticket's
// slots cannot be recycled meanwhile: only the ticket's own wait call releases them.
int presync_pkg(lsg_ctx* c, lsg_ticket t, bool partial_only) {
  std::vector<std::pair<int, hipEvent_t>> evs;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const int p = ticket_pkg(c, t);
    if (p < 0) return LSG_ERR_INVALID_ARG;
    for (int d = 0; d < c->n_dev; d++) {
      Slot* s = &c->dev[d]->slots[p];
      evs.push_back({c->dev[d]->device, partial_only ? s->ev_part : s->ev_done});
    }
  }
  for (auto& e : evs) {
    (void)hipSetDevice(e.first);
    hipError_t r = event_wait(e.second);
    if (r != hipSuccess) {
      std::lock_guard<std::mutex> lk(c->mu);
      return fail_c(c, "hipEventSynchronize", r);
    }
  }
  return LSG_OK;
}

// ---- final-exponentiation entries (device 0): ng groups of pg partials
int submit_final(Slot* s, const uint8_t* partials576, size_t ng, size_t pg, bool on_device = false) {
  timer_reset(s);
  s->plan.clear();
  const size_t n = ng * pg, np = std::max(n, (size_t)1), gq = std::max(ng, (size_t)1);
  LSG_RC(ensure_host(s, s->h_blob, 576 * np));
  LSG_RC(ensure(s, s->d_Fb, 576 * std::max(np, gq)));
  LSG_RC(ensure(s, s->d_aux, 4 * W_F12 * np));
  LSG_RC(ensure(s, s->d_F, 4 * W_F12 * gq));
  LSG_RC(ensure(s, s->d_verdict, 4 * gq));
  LSG_RC(ensure_host(s, s->h_verdict, 4 * gq));
  s->n_sets = ng;  // verdict count
  if (n) {
    std::vector<int32_t> off, len;
    for (size_t g = 0; g < ng; g++) {
      off.push_back((int32_t)(g * pg));
      len.push_back((int32_t)pg);
    }
    SegPlan P = slot_seg(s, 2, off, len, false, 0, 0);
    LSG_RC(upload_plan(s));
    hipStream_t S = s->st[0];
    if (on_device) {  // the caller's device buffer (e.g. a collective's output): no host copy
      LSG_HIP(s, hipMemcpyAsync(s->d_Fb.p, partials576, 576 * n, hipMemcpyDeviceToDevice, S));
    } else {
      memcpy(s->h_blob.p, partials576, 576 * n);
      LSG_HIP(s, hipMemcpyAsync(s->d_Fb.p, s->h_blob.p, 576 * n, hipMemcpyHostToDevice, S));
    }
    KL(s, "k_blobs_to_fp12", lsgk::blobs_to_fp12(S, (int)n, P_<uint8_t>(s->d_Fb), P_<uint32_t>(s->d_aux)));
    LSG_RC(run_seg(s, 2, "fp12_product", P, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_F)));
    KL(s, "k_fp12_to_canon", lsgk::fp12_to_canon(S, (int)ng, P_<uint32_t>(s->d_F), P_<uint8_t>(s->d_Fb)));
    KL(s, "slp_final_exp", lsg_slp_final_exp(S, (int)ng, P_<uint8_t>(s->d_Fb), P_<int32_t>(s->d_verdict)));
    LSG_HIP(s, hipMemcpyAsync(s->h_verdict.p, s->d_verdict.p, 4 * ng, hipMemcpyDeviceToHost, S));
  } else {
    s->n_sets = 0;
  }
  LSG_HIP(s, hipEventRecord(s->ev_done, s->st[0]));
  return LSG_OK;
}

// stage + expand + hash on the utility slot (synchronous callers only)
int util_hash(Slot* s, const uint8_t* msgs, uint32_t msg_len, size_t n, const uint8_t* dst, uint32_t dst_len) {
  std::vector<lsg_set> sets(n);
  std::vector<const lsg_set*> sp(n);
  for (size_t i = 0; i < n; i++) {
    memset(&sets[i], 0, sizeof(lsg_set));
    sets[i].msg = msgs + (size_t)msg_len * i;
    sets[i].msg_len = msg_len;
    sp[i] = &sets[i];
  }
  LSG_RC(stage_sets(s, sp.data(), n, 0, false));
  LSG_RC(size_state(s, n, 0, 1, 0));
  LSG_HIP(s, hipMemcpyAsync(s->d_dst.p, dst, dst_len, hipMemcpyHostToDevice, s->st[0]));
  const int nn = (int)n;
  KL(s, "k_expand_msg", lsgk::expand_msg(S_(s), nn, P_<uint8_t>(s->d_msg), P_<uint32_t>(s->d_msgoff),
                                         P_<uint32_t>(s->d_msglen), P_<uint8_t>(s->d_dst), dst_len, P_<uint8_t>(s->d_ub)));
  LSG_RC(launch_hash(s, nn, P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf)));
  // the utility slot's DST is restored for the next caller
  LSG_HIP(s, hipMemcpyAsync(s->d_dst.p, DST_POP, DST_POP_LEN, hipMemcpyHostToDevice, s->st[0]));
  return LSG_OK;
}

// keys (one "set" of n keys) into the utility slot's arena, decoded on its stream
int util_stage_keys(Slot* s, const uint8_t* pks, uint32_t pk_len, size_t n) {
  lsg_set q;
  memset(&q, 0, sizeof(q));
  q.pks = pks;
  q.pk_len = pk_len;
  q.n_pks = (uint32_t)n;
  const lsg_set* qp = &q;
  LSG_RC(stage_sets(s, &qp, 1, 0, false));
  return size_state(s, 1, n, 1, 0);
}

int dev_create(lsg_ctx* c, int ord, int device, Dev** out) {
  Dev* d = new Dev();
  *out = d;
  d->c = c;
  d->device = device;
  d->ord = ord;
  LSG_HIPC(c, hipSetDevice(device));
  LSG_HIPC(c, hipStreamCreateWithFlags(&d->s_util, hipStreamNonBlocking));
  // pipeline slots are created on first use (slot_ready): 64 x 2 streams per device up front
  // would cost init time nobody needs below a few packages in flight
  if (ord == 0) {
    for (int i = 0; i < LSG_FE_STREAMS; i++) LSG_HIPC(c, hipStreamCreateWithFlags(&d->s_fe[i], hipStreamNonBlocking));
    for (int i = 0; i < LSG_FINALS; i++) LSG_RC(slot_create(d, &d->finals[i], i, d->s_fe[i % LSG_FE_STREAMS]));
  }
  return slot_create(d, &d->util, 0, d->s_util);
}

void dev_destroy(Dev* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  for (Slot& s : d->slots) slot_destroy(&s);
  for (Slot& s : d->finals) slot_destroy(&s);
  slot_destroy(&d->util);
  free_dev(d->d_pktab);
  free_dev(d->d_pktab_ok);
  free_dev(d->d_cm_idx);
  free_dev(d->d_cm_off);
  free_dev(d->d_cm_sum);
  free_dev(d->d_dep_in);
  free_dev(d->d_dep_roots);
  free_dev(d->d_mc_rows);
  free_dev(d->d_mc_inf);
  if (d->s_util) (void)hipStreamDestroy(d->s_util);
  for (hipStream_t st : d->s_fe)
    if (st) (void)hipStreamDestroy(st);
  if (d->s_xp) (void)hipStreamDestroy(d->s_xp);
  if (d->s_nfe) (void)hipStreamDestroy(d->s_nfe);
  for (hipStream_t st : d->s_pp)
    if (st) (void)hipStreamDestroy(st);
  delete d;
}

// pubkey table rows first .. first+n-1 on one device
int dev_pktab_set(Dev* d, size_t first, const uint8_t* pks, uint32_t pk_len, size_t n, std::vector<int32_t>& pkerr) {
  lsg_ctx* c = d->c;
  Slot* s = &d->util;
  timer_reset(s);
  LSG_HIPC(c, hipSetDevice(d->device));
  const size_t need = first + n;
  // tickets in flight read the table: drain the device before moving it or rewriting rows
  // that may be read (an in-flight aggregate must never see a half-written row)
  if (need > d->pktab_cap || first < d->pktab_n) LSG_HIPC(c, hipDeviceSynchronize());
  if (need > d->pktab_cap) {
    const size_t cap = std::max(std::max(need, 2 * d->pktab_cap), (size_t)1024);
    DevBuf nt, nok;
    LSG_HIPC(c, hipMalloc(&nt.p, 4 * W_TAB * cap));
    g_allocs++;
    nt.cap = 4 * W_TAB * cap;
    hipError_t e = hipMalloc(&nok.p, cap);
    if (e != hipSuccess) {
      free_dev(nt);
      return fail_c(c, "hipMalloc", e);
    }
    g_allocs++;
    nok.cap = cap;
    LSG_HIPC(c, hipMemset(nok.p, 0, cap));
    if (d->pktab_n) {
      LSG_HIPC(c, hipMemcpy(nt.p, d->d_pktab.p, 4 * W_TAB * d->pktab_n, hipMemcpyDeviceToDevice));
      LSG_HIPC(c, hipMemcpy(nok.p, d->d_pktab_ok.p, d->pktab_n, hipMemcpyDeviceToDevice));
    }
    free_dev(d->d_pktab);
    free_dev(d->d_pktab_ok);
    d->d_pktab = nt;
    d->d_pktab_ok = nok;
    d->pktab_cap = cap;
  }
  LSG_RC(util_stage_keys(s, pks, pk_len, n));
  // decode straight into the table rows first .. first + n - 1: affine points (the first
  // level of the aggregation tree reads them as they are), row flag 1 = a finite key, 2 = the
  // infinity key, 0 = no key
  LSG_RC(ensure(s, s->d_ub, n));
  KL(s, "k_pk_gather_aff", lsgk::pk_gather_aff(S_(s), (int)n, P_<uint8_t>(s->d_pk), s->pk_stride,
                                               P_<uint32_t>(s->d_pklen), P_<uint32_t>(d->d_pktab) + W_TAB * first,
                                               P_<uint8_t>(s->d_ub), P_<int32_t>(s->d_pkerr), nullptr, nullptr, 0u));
  pkerr.assign(n, 0);
  std::vector<uint8_t> inf(n);
  LSG_HIP(s, hipMemcpyAsync(pkerr.data(), s->d_pkerr.p, 4 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(inf.data(), s->d_ub.p, n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  std::vector<uint8_t> ok(n);
  for (size_t k = 0; k < n; k++) ok[k] = pkerr[k] != 0 ? 0 : (inf[k] ? 2 : 1);
  LSG_HIP(s, hipMemcpy(P_<uint8_t>(d->d_pktab_ok) + first, ok.data(), n, hipMemcpyHostToDevice));
  d->pktab_n = std::max(d->pktab_n, need);
  keep_times(s);
  return LSG_OK;
}

}  // namespace

// ---------------------------------------------------------------------------- C ABI
extern "C" {

int lsg_init_devices(const int* device_ids, int n_devices, lsg_ctx** out) {
  if (!out || !device_ids || n_devices < 1 || n_devices > LSG_MAX_DEVICES) return LSG_ERR_INVALID_ARG;
  *out = nullptr;
  // A package keeps two streams busy and up to LSG_SLOTS packages are in flight: HIP's default
  // of 4 hardware queues per process serialises them (profiles/r05_hwq_ab.txt).  The library
  // owns this setting: before its first HIP call it sets GPU_MAX_HW_QUEUES to LSG_HW_QUEUES
  // (1..32, default LSG_DEFAULT_HW_QUEUES), overriding a process-wide default such as the
  // GPU_MAX_HW_QUEUES=4 some hosts export.  It takes effect when HIP is not yet initialised --
  // the first lsg_init of a Node process; INTEGRATION.md section 5.
  // setenv is not safe against getenv on other threads: a host calls lsg_init before it
  // starts threads that read the environment.  A value already in the
  // environment is replaced, and said so once: if HIP was initialised before (by another
  // library), the replacement comes too late to take effect.
  static std::once_flag hwq_once;
  std::call_once(hwq_once, [] {
    const char* want = getenv("LSG_HW_QUEUES");
    const int q = want ? atoi(want) : 0;
    const char* v = (q >= 1 && q <= 32) ? want : LSG_DEFAULT_HW_QUEUES;
    const char* had = getenv("GPU_MAX_HW_QUEUES");
    if (had && strcmp(had, v) != 0)
      fprintf(stderr, "lodestar_bls: GPU_MAX_HW_QUEUES=%s replaced by %s (LSG_HW_QUEUES); effective unless HIP was "
                      "initialised earlier in this process\n", had, v);
    setenv("GPU_MAX_HW_QUEUES", v, 1);
  });
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return LSG_ERR_NO_DEVICE;
  bool distinct = true;
  for (int i = 0; i < n_devices; i++) {
    const int dev = device_ids[i];
    if (dev < 0 || dev >= count) return LSG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return LSG_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return LSG_ERR_NO_DEVICE;
    for (int j = 0; j < i; j++)
      if (device_ids[j] == dev) distinct = false;
  }
  lsg_ctx* c = new lsg_ctx();
  c->n_dev = n_devices;
  int rc = LSG_OK;
  for (int i = 0; i < n_devices && !rc; i++) rc = dev_create(c, i, device_ids[i], &c->dev[i]);
  if (!rc && distinct && (n_devices > 1 || force_exchange())) {
    // the partial exchange of SURVEY.md 8e: one RCCL communicator per device, owned here
    ncclResult_t r = ncclCommInitAll(c->comm, n_devices, device_ids);
    if (r != ncclSuccess) {
      c->err = std::string("ncclCommInitAll: ") + ncclGetErrorString(r);
      rc = LSG_ERR_DEVICE;
    } else {
      c->rccl = true;
    }
  }
  (void)hipSetDevice(device_ids[0]);
  if (rc) {
    lsg_destroy(c);
    return rc;
  }
  *out = c;
  return LSG_OK;
}

int lsg_init(int device_ordinal, lsg_ctx** out) {
  const int dev = device_ordinal < 0 ? 0 : device_ordinal;
  return lsg_init_devices(&dev, 1, out);
}

int lsg_destroy(lsg_ctx* c) {
  if (!c) return LSG_ERR_INVALID_ARG;
  for (int d = 0; d < c->n_dev; d++) dev_destroy(c->dev[d]);
  if (c->rccl)
    for (int d = 0; d < c->n_dev; d++)
      if (c->comm[d]) (void)ncclCommDestroy(c->comm[d]);
  delete c;
  return LSG_OK;
}

int lsg_device_count(lsg_ctx* c, int32_t* n) {
  if (!c || !n) return LSG_ERR_INVALID_ARG;
  *n = c->n_dev;
  return LSG_OK;
}

// a copy per calling thread: another thread's failing call may replace c->err meanwhile
const char* lsg_last_error(lsg_ctx* c) {
  if (!c) return "null context";
  thread_local std::string copy;
  std::lock_guard<std::mutex> lk(c->mu);
  copy = c->err;
  return copy.c_str();
}

int lsg_device_name(lsg_ctx* c, char* buf, size_t len) {
  if (!c || !buf || !len) return LSG_ERR_INVALID_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->dev[0]->device) != hipSuccess) return LSG_ERR_DEVICE;
  snprintf(buf, len, "%s (%s, %d CUs)%s", prop.name, prop.gcnArchName, prop.multiProcessorCount,
           c->n_dev > 1 ? " x several" : "");
  return LSG_OK;
}

int lsg_reserve(lsg_ctx* c, size_t max_sets, size_t max_pks, size_t max_msg_bytes, int32_t n_slots) {
  if (!c || n_slots < 0) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  const int ns = std::min(n_slots == 0 ? LSG_SLOTS : n_slots, LSG_SLOTS);
  if (c->n_dev > 1) {
    // a device stages its share of a package: whole jobs by cumulative set count (assign_jobs),
    // so at most 1/n of the sets plus one job's -- reserved with a job's worth of slack (a larger
    // share grows its slot's buffers when it comes)
    const size_t n = (size_t)c->n_dev;
    max_sets = std::min(max_sets, max_sets / n + 4096);
    max_pks = std::min(max_pks, max_pks / n + 4096 * 512);
    max_msg_bytes = std::min(max_msg_bytes, max_msg_bytes / n + 4096 * 32);
  }
  for (int d = 0; d < c->n_dev; d++) {
    LSG_HIPC(c, hipSetDevice(c->dev[d]->device));
    for (int i = 0; i < ns; i++) {
      Slot* s = &c->dev[d]->slots[i];
      if (s->kind != SLOT_FREE) continue;
      LSG_RC(slot_ready(c->dev[d], s, i));
      LSG_RC(size_inputs(s, max_sets, max_pks, max_msg_bytes));
      // groups: as many as sets (the per-job phase of a failing package of single-set jobs)
      LSG_RC(size_state(s, max_sets, max_pks, max_sets, max_sets / 256 + 1, 1));
      // the bit arena of committee + bits sets, once the context has committees (a context that
      // never registers one reserves what it did before): a bits set of n bits counts
      // 16 + ceil(n / 32) toward max_pks, which covers its 4 ceil(n / 32) arena bytes here and
      // its plan words (6 + up to 32 lane pairs) below; a multi-committee set of n bits over k
      // committees counts 16 + 2 k + ceil(n / 32): at most ceil(n / 32) + k arena words, and
      // 5 + 4 k plan words + up to 32 lane pairs
      if (!c->cm_ok.empty()) {
        LSG_RC(ensure_host(s, s->h_cbits, 4 * max_pks));
        LSG_RC(ensure(s, s->d_cbits, 4 * max_pks));
      }
      // the group buffers of lsg_submit_jobs_grouped (max_sets sets in max_sets groups), once the
      // context has seen a grouped package: the caller reserves again after its first one
      if (c->grouped_seen) {
        LSG_RC(size_groups(s, max_sets, max_sets));
        s->set_grp.reserve(max_sets);
      }
      // the message cache's per-slot buffers, once the context has one (lsg_msg_cache_set; as the
      // bit arena above): the misses' points beside the per-message ones, which such a package
      // always has -- its message table is always built -- with the per-message key sums
      if (c->dev[d]->mc.capacity()) {
        const size_t nn = std::max(max_sets, (size_t)1);
        LSG_RC(ensure(s, s->d_Hx, 4 * W_G2A * nn));
        LSG_RC(ensure(s, s->d_hinfx, nn));
        LSG_RC(ensure(s, s->d_Hm, 4 * W_G2A * nn));
        LSG_RC(ensure(s, s->d_hinfm, nn));
        LSG_RC(ensure(s, s->d_mmask, 4 * W_G1P * nn));
        LSG_RC(ensure(s, s->d_PmP, 4 * W_G1P * nn));
        LSG_RC(ensure(s, s->d_Pm, 4 * W_G1A * nn));
        LSG_RC(ensure(s, s->d_pinfm, nn));
        LSG_RC(ensure(s, s->d_errm, 4 * nn));
        s->mc_pins.reserve(max_sets);
        s->mc_pend.reserve(max_sets);
        s->mc_store.reserve(2 * max_sets);
      }
      LSG_RC(ensure_host(s, s->h_mode, std::max(max_sets, (size_t)1)));
      const size_t plan_words = 16 * max_sets + 4 * max_pks + 64 * 1024;
      LSG_RC(ensure_host(s, s->h_plan, 4 * plan_words));
      LSG_RC(ensure(s, s->d_plan, 4 * plan_words));
      s->plan.reserve(plan_words);
      for (int u = 0; u < 3; u++) {
        const size_t W = u == 0 ? W_G1P : (u == 1 ? W_G2P : W_F12);
        const size_t items = std::max(max_sets / 8 + 64, std::max(max_pks, max_sets) / 8 + 64);
        for (int k = 0; k < 2; k++) LSG_RC(ensure(s, s->seg_tmp[u][k], 4 * W * items));
      }
      // timing events for a full submission, created up front
      while (s->timers.size() < 192) {
        Timer t;
        LSG_HIPC(c, hipEventCreate(&t.a));
        LSG_HIPC(c, hipEventCreate(&t.b));
        s->timers.push_back(t);
      }
    }
  }
  LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
  return LSG_OK;
}

int lsg_allocation_count(lsg_ctx* c, uint64_t* n) {
  if (!c || !n) return LSG_ERR_INVALID_ARG;
  *n = g_allocs.load();
  return LSG_OK;
}

int lsg_submit_jobs(lsg_ctx* c, const lsg_job* jobs, size_t n_jobs, uint64_t seed, lsg_ticket* ticket) {
  if (!c || !ticket || (n_jobs && !jobs)) return LSG_ERR_INVALID_ARG;
  for (size_t j = 0; j < n_jobs; j++)
    if (jobs[j].n_sets && !jobs[j].sets) return LSG_ERR_INVALID_ARG;
  // an LSG_MSG_OBJECT set that selects no kind or has no bytes is a caller bug, refused before a
  // slot is taken (lsg_verify_jobs and lsg_verify_sets come through here)
  if (!msg_jobs_ok(jobs, n_jobs)) return LSG_ERR_INVALID_ARG;
  CtxLock lk(c->mu);
  LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
  bool prio = false;
  for (size_t j = 0; j < n_jobs; j++) prio = prio || (jobs[j].flags & LSG_JOB_PRIORITY) != 0;
  if (c->co_max_sets && c->n_dev == 1 && !prio) {  // (a priority package is never held back)
    size_t ns = 0;
    for (size_t j = 0; j < n_jobs; j++) ns += jobs[j].n_sets;
    if (ns <= c->co_max_sets) return submit_merged(c, jobs, n_jobs, seed, ns, ticket);
  }
  return submit_pkg(c, lk, jobs, n_jobs, seed, ticket);
}

int lsg_set_coalesce(lsg_ctx* c, uint32_t max_sets, int32_t max_inflight) {
  if (!c || max_inflight < 1) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  LSG_RC(flush_pending(c));
  c->co_max_sets = max_sets;
  c->co_inflight = max_inflight;
  return LSG_OK;
}

// A grouped package launches on its own, as the packages of
// lsg_verify_deposits do: never held by lsg_set_coalesce, and it flushes nothing that holds.
int lsg_submit_jobs_grouped(lsg_ctx* c, const lsg_job* jobs, size_t n_jobs, uint64_t seed, const uint32_t* set_group,
                            size_t n_groups, lsg_ticket* ticket) {
  if (!set_group || n_groups == 0) return lsg_submit_jobs(c, jobs, n_jobs, seed, ticket);
  if (!c || !ticket || (n_jobs && !jobs) || n_groups > 0x7fffffffull) return LSG_ERR_INVALID_ARG;
  size_t ns = 0;
  for (size_t j = 0; j < n_jobs; j++) {
    if (jobs[j].n_sets && !jobs[j].sets) return LSG_ERR_INVALID_ARG;
    ns += jobs[j].n_sets;
  }
  if (!msg_jobs_ok(jobs, n_jobs)) return LSG_ERR_INVALID_ARG;
  CtxLock lk(c->mu);
  for (size_t i = 0; i < ns; i++)
    if (set_group[i] != LSG_NO_GROUP && set_group[i] >= n_groups) {
      c->err = "lsg_submit_jobs_grouped: set " + std::to_string(i) + " names group " + std::to_string(set_group[i]) +
               " of " + std::to_string(n_groups);
      return LSG_ERR_INVALID_ARG;
    }
  if (c->n_dev > 1) {
    c->err = "lsg_submit_jobs_grouped: groups are single-device (a group can span devices)";
    return LSG_ERR_INVALID_ARG;
  }
  LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
  c->grouped_seen = true;
  return submit_pkg(c, lk, jobs, n_jobs, seed, ticket, true, nullptr, set_group, n_groups);
}

static int wait_jobs_impl(lsg_ctx* c, lsg_ticket ticket, int32_t node_valid, lsg_job_result* results, lsg_stats* stats,
                          uint8_t* agg96, uint32_t* agg_n);

int lsg_wait_jobs_grouped(lsg_ctx* c, lsg_ticket ticket, lsg_job_result* results, lsg_stats* stats, uint8_t* agg96,
                          uint32_t* agg_n) {
  return wait_jobs_impl(c, ticket, -1, results, stats, agg96, agg_n);
}

int lsg_wait_jobs_node(lsg_ctx* c, lsg_ticket ticket, int32_t node_valid, lsg_job_result* results, lsg_stats* stats) {
  return wait_jobs_impl(c, ticket, node_valid, results, stats, nullptr, nullptr);
}

static int wait_jobs_impl(lsg_ctx* c, lsg_ticket ticket, int32_t node_valid, lsg_job_result* results, lsg_stats* stats,
                          uint8_t* agg96, uint32_t* agg_n) {
  if (!c) return LSG_ERR_INVALID_ARG;
  if (((ticket >> 8) & 255) == SLOT_MERGE) {
    if (node_valid != -1) {
      c->err = "lsg_wait_jobs_node: a coalesced package has no node check of its own";
      return LSG_ERR_INVALID_ARG;
    }
    if (!results) return LSG_ERR_INVALID_ARG;
    return wait_merged(c, ticket, results, stats);
  }
  if (int prc = presync_pkg(c, ticket, false)) return prc;
  CtxLock lk(c->mu);
  LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
  const int p = ticket_pkg(c, ticket);
  if (p < 0) return LSG_ERR_INVALID_ARG;
  const size_t nj = c->dev[0]->slots[p].n_jobs;
  if (nj && !results) return LSG_ERR_INVALID_ARG;
  if (node_valid != -1 && c->n_dev > 1) {
    c->err = "lsg_wait_jobs_node: a multi-device context runs its own node check";
    return LSG_ERR_INVALID_ARG;
  }
  const int rc = wait_pkg(c, &lk, p, node_valid == -1 ? -2 : (node_valid ? 1 : 0), results, stats, agg96, agg_n);
  maybe_flush(c);
  return rc;
}

int lsg_wait_jobs(lsg_ctx* c, lsg_ticket ticket, lsg_job_result* results, lsg_stats* stats) {
  return lsg_wait_jobs_node(c, ticket, -1, results, stats);
}

int lsg_jobs_partial(lsg_ctx* c, lsg_ticket ticket, uint8_t* out576, int32_t* has_batch) {
  if (!c || !out576) return LSG_ERR_INVALID_ARG;
  if (c->n_dev > 1) {
    c->err = "lsg_jobs_partial: a multi-device context exchanges its partials itself";
    return LSG_ERR_INVALID_ARG;
  }
  if (int prc = presync_pkg(c, ticket, true)) return prc;
  LSG_ENTER(c);
  const int p = ticket_pkg(c, ticket);
  if (p < 0) return LSG_ERR_INVALID_ARG;
  Slot* s = &c->dev[0]->slots[p];
  const bool has = !s->phA.groups.empty() && s->gp.big_g >= 0;
  if (has && s->gp.lone_unscaled) {
    const uint8_t* src;
    LSG_RC(export_partial_dev(s, &src));
    LSG_RC(ensure_host(s, s->h_xport, 576));
    LSG_HIP(s, hipMemcpyAsync(s->h_xport.p, src, 576, hipMemcpyDeviceToHost, s->st[0]));
    LSG_HIP(s, hipStreamSynchronize(s->st[0]));
    memcpy(out576, s->h_xport.p, 576);
  } else if (has) {
    memcpy(out576, H_<uint8_t>(s->h_blob) + 576 * (size_t)s->gp.big_g, 576);
  } else {
    memcpy(out576, fp12_one_blob(), 576);
  }
  if (has_batch) *has_batch = has ? 1 : 0;
  return LSG_OK;
}

int lsg_jobs_partial_device(lsg_ctx* c, lsg_ticket ticket, void* dev_out576, int32_t* has_batch) {
  if (!c || !dev_out576) return LSG_ERR_INVALID_ARG;
  if (c->n_dev > 1) {
    c->err = "lsg_jobs_partial_device: a multi-device context exchanges its partials itself";
    return LSG_ERR_INVALID_ARG;
  }
  if (int prc = presync_pkg(c, ticket, true)) return prc;
  hipEvent_t xev;
  bool has;
  {
    LSG_ENTER(c);
    const int p = ticket_pkg(c, ticket);
    if (p < 0) return LSG_ERR_INVALID_ARG;
    Slot* s = &c->dev[0]->slots[p];
    has = !s->phA.groups.empty() && s->gp.big_g >= 0;
    // the copy goes out on a high-priority stream (the node final exponentiations'): on the
    // package's own stream it would queue behind other packages' kernels sharing its hardware
    // queue, and the node's next verdicts wait on it (ev_part is complete: presync_pkg)
    LSG_RC(prio_stream(c, c->dev[0], &c->dev[0]->s_xp));
    hipStream_t xs = c->dev[0]->s_xp;
    if (has) {
      const uint8_t* src;
      LSG_RC(export_partial_dev(s, &src, xs));  // f^r (a lone unscaled set) runs on xs too
      LSG_HIP(s, hipMemcpyAsync(dev_out576, src, 576, hipMemcpyDeviceToDevice, xs));
    } else {
      LSG_HIP(s, hipMemcpyAsync(dev_out576, fp12_one_blob(), 576, hipMemcpyHostToDevice, xs));
    }
    LSG_HIP(s, hipEventRecord(s->ev_xp, xs));
    xev = s->ev_xp;  // (the slot stays this ticket's until it is waited on)
  }
  // the copy completes without the context lock held: submissions and resolutions of other
  // packages go on meanwhile
  (void)hipSetDevice(c->dev[0]->device);
  if (hipError_t e = event_wait(xev)) {
    std::lock_guard<std::mutex> lk(c->mu);  // (c->err is written under the lock)
    return fail_c(c, "hipEventSynchronize", e);
  }
  if (has_batch) *has_batch = has ? 1 : 0;
  return LSG_OK;
}

int lsg_verify_jobs(lsg_ctx* c, const lsg_job* jobs, size_t n_jobs, uint64_t seed, lsg_job_result* results,
                    lsg_stats* stats) {
  if (!c || (n_jobs && (!jobs || !results))) return LSG_ERR_INVALID_ARG;
  lsg_ticket t;
  int rc = lsg_submit_jobs(c, jobs, n_jobs, seed, &t);
  if (rc) return rc;
  return lsg_wait_jobs(c, t, results, stats);
}

int lsg_verify_sets(lsg_ctx* c, const lsg_set* sets, size_t n_sets, uint64_t seed, lsg_job_result* result) {
  if (!c || !result || (n_sets && !sets)) return LSG_ERR_INVALID_ARG;
  lsg_job job;
  job.sets = sets;
  job.n_sets = (uint32_t)n_sets;
  job.flags = 0;
  return lsg_verify_jobs(c, &job, 1, seed, result, nullptr);
}

int lsg_pipeline_slots(lsg_ctx* c, int32_t* n) {
  if (!c || !n) return LSG_ERR_INVALID_ARG;
  *n = LSG_SLOTS;
  return LSG_OK;
}

int lsg_poll(lsg_ctx* c, lsg_ticket ticket, int32_t* done) {
  if (!c || !done) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  std::vector<hipEvent_t> evs;
  std::vector<Slot*> mcs;
  if (Slot* f = ticket_final(c, ticket)) {
    evs.push_back(f->ev_done);
  } else if (((ticket >> 8) & 255) == SLOT_MERGE) {
    auto it = c->merged.find(ticket >> 16);
    if (it == c->merged.end()) return LSG_ERR_INVALID_ARG;
    if (it->second.rc) {  // its launch failed: done (the wait reports the failure)
      *done = 1;
      return LSG_OK;
    }
    if (it->second.slot < 0) {  // not launched: launch when the device has room
      maybe_flush(c);
      it = c->merged.find(ticket >> 16);
      if (it == c->merged.end()) return LSG_ERR_INVALID_ARG;
      if (it->second.slot < 0) {
        *done = it->second.rc ? 1 : 0;
        return LSG_OK;
      }
    }
    evs.push_back(c->dev[0]->slots[it->second.slot].ev_done);
    mcs.push_back(&c->dev[0]->slots[it->second.slot]);
  } else {
    const int p = ticket_pkg(c, ticket);
    if (p < 0) return LSG_ERR_INVALID_ARG;
    for (int d = 0; d < c->n_dev; d++) {
      evs.push_back(c->dev[d]->slots[p].ev_done);
      mcs.push_back(&c->dev[d]->slots[p]);
    }
  }
  *done = 1;
  for (hipEvent_t e : evs) {
    hipError_t r = hipEventQuery(e);
    if (r == hipErrorNotReady) {
      *done = 0;
      return LSG_OK;
    }
    if (r != hipSuccess) return fail_c(c, "hipEventQuery", r);
  }
  for (Slot* s : mcs) mc_settle(s, true);  // completion observed: the launch's cache rows become visible
  return LSG_OK;
}

// one shard's partial (sync): all sets as one batchable job.  rnd_in: the
// randomizers of lsg_check_batch_partial_rnd in place of the seed's draws
static int batch_partial(lsg_ctx* c, const lsg_set* sets, size_t n_sets, uint64_t seed, const uint64_t* rnd_in,
                         uint8_t* out576, int32_t* set_err, int32_t* any_error) {
  if (!c || !out576 || !any_error || (n_sets && !sets)) return LSG_ERR_INVALID_ARG;
  if (c->n_dev > 1) {
    c->err = "lsg_batch_partial: single-device contexts only";
    return LSG_ERR_INVALID_ARG;
  }
  if (!msg_sets_ok(sets, n_sets)) return LSG_ERR_INVALID_ARG;
  lsg_ticket t;
  {
    CtxLock lk(c->mu);
    LSG_HIPC(c, hipSetDevice(c->dev[0]->device));
    lsg_job job;
    job.sets = sets;
    job.n_sets = (uint32_t)n_sets;
    job.flags = LSG_JOB_BATCHABLE;
    // the partial leaves: every r_i random
    // (outside the message cache: this call frees its slot itself)
    int rc = submit_pkg(c, lk, &job, 1, seed, &t, false, nullptr, nullptr, 0, rnd_in, false);
    if (rc) return rc;
  }
  const int prc = presync_pkg(c, t, false);
  LSG_ENTER(c);
  const int p = ticket_pkg(c, t);
  if (p < 0) return LSG_ERR_INVALID_ARG;
  Slot* s = &c->dev[0]->slots[p];
  if (prc) {  // the internal ticket cannot be waited on again: give its slot back
    sync_slot(s);
    s->kind = SLOT_FREE;
    return prc;
  }
  const SetStatus ss = read_status(s);
  *any_error = 0;
  for (size_t i = 0; i < n_sets; i++) {
    int32_t e = set_error(ss, i);
    if (!s->shape.bits_kerr.empty() && s->shape.bits_kerr[i]) e = s->shape.bits_kerr[i];
    if (set_err) set_err[i] = e;
    if (e) *any_error = 1;
  }
  for (size_t k = 0; k < s->n_pks; k++)
    if (ss.pkerr[k]) *any_error = 1;
  if (s->gp.big_g >= 0)
    memcpy(out576, H_<uint8_t>(s->h_blob) + 576 * (size_t)s->gp.big_g, 576);
  else
    memcpy(out576, fp12_one_blob(), 576);
  s->kind = SLOT_FREE;
  keep_times(s);
  return LSG_OK;
}

int lsg_batch_partial(lsg_ctx* c, const lsg_set* sets, size_t n_sets, uint64_t seed, uint8_t* out576,
                      int32_t* set_err, int32_t* any_error) {
  return batch_partial(c, sets, n_sets, seed, nullptr, out576, set_err, any_error);
}

// parity hook (tests): lsg_batch_partial with the caller's randomizers; every argument error is
// reported before anything is staged
int lsg_check_batch_partial_rnd(lsg_ctx* c, const lsg_set* sets, size_t n_sets, const uint64_t* rnd, uint8_t* out576,
                                int32_t* set_err, int32_t* any_error) {
  if (!c || !out576 || !any_error || (n_sets && (!sets || !rnd))) return LSG_ERR_INVALID_ARG;
  for (size_t i = 0; i < n_sets; i++)
    if (rnd[i] == 0) return LSG_ERR_INVALID_ARG;
  return batch_partial(c, sets, n_sets, 1, rnd, out576, set_err, any_error);
}

int lsg_final_submit_groups(lsg_ctx* c, const uint8_t* partials576, size_t n_groups, size_t per_group,
                            lsg_ticket* ticket) {
  if (!c || !ticket || (n_groups && per_group && !partials576) || (n_groups && !per_group)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = nullptr;
  for (int i = 0; i < LSG_FINALS && !s; i++)
    if (c->dev[0]->finals[i].kind == SLOT_FREE) s = &c->dev[0]->finals[i];
  if (!s) {
    c->err = "all final-exponentiation entries are busy";
    return LSG_ERR_BUSY;
  }
  // a node verdict waits on this one program: the greatest stream priority (the entry is free)
  LSG_RC(prio_stream(c, c->dev[0], &c->dev[0]->s_nfe));
  s->st[0] = s->st[1] = c->dev[0]->s_nfe;
  int rc = submit_final(s, partials576, n_groups, per_group);
  if (rc) {
    sync_slot(s);
    return rc;
  }
  uint64_t serial;
  *ticket = make_ticket(c, SLOT_FINAL, s->index, &serial);
  s->kind = SLOT_FINAL;
  s->serial = serial;
  return LSG_OK;
}

int lsg_final_submit_device(lsg_ctx* c, const void* dev_partials576, size_t n_partials, lsg_ticket* ticket) {
  if (!c || !ticket || (n_partials && !dev_partials576)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = nullptr;
  for (int i = 0; i < LSG_FINALS && !s; i++)
    if (c->dev[0]->finals[i].kind == SLOT_FREE) s = &c->dev[0]->finals[i];
  if (!s) {
    c->err = "all final-exponentiation entries are busy";
    return LSG_ERR_BUSY;
  }
  LSG_RC(prio_stream(c, c->dev[0], &c->dev[0]->s_nfe));
  s->st[0] = s->st[1] = c->dev[0]->s_nfe;
  int rc = submit_final(s, (const uint8_t*)dev_partials576, n_partials ? 1 : 0, n_partials, true);
  if (rc) {
    sync_slot(s);
    return rc;
  }
  uint64_t serial;
  *ticket = make_ticket(c, SLOT_FINAL, s->index, &serial);
  s->kind = SLOT_FINAL;
  s->serial = serial;
  return LSG_OK;
}

int lsg_final_submit(lsg_ctx* c, const uint8_t* partials576, size_t n_partials, lsg_ticket* ticket) {
  if (!c || !ticket || (n_partials && !partials576)) return LSG_ERR_INVALID_ARG;
  return lsg_final_submit_groups(c, partials576, n_partials ? 1 : 0, n_partials, ticket);
}

static int final_wait(lsg_ctx* c, lsg_ticket ticket, int32_t* valid, bool single) {
  if (!c || !valid) return LSG_ERR_INVALID_ARG;
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    Slot* s = ticket_final(c, ticket);
    if (!s) return LSG_ERR_INVALID_ARG;
    ev = s->ev_done;
  }
  (void)hipSetDevice(c->dev[0]->device);
  hipError_t e = event_wait(ev);
  LSG_ENTER(c);
  if (e != hipSuccess) return fail_c(c, "hipEventSynchronize", e);
  Slot* s = ticket_final(c, ticket);
  if (!s) return LSG_ERR_INVALID_ARG;
  if (single && s->n_sets > 1) {
    c->err = "ticket carries several groups: use lsg_final_wait_groups";
    return LSG_ERR_INVALID_ARG;
  }
  if (!s->n_sets) valid[0] = 0;
  for (size_t g = 0; g < s->n_sets; g++) valid[g] = H_<int32_t>(s->h_verdict)[g];
  s->kind = SLOT_FREE;
  keep_times(s);
  return LSG_OK;
}

int lsg_final_wait_groups(lsg_ctx* c, lsg_ticket ticket, int32_t* valid) { return final_wait(c, ticket, valid, false); }
int lsg_final_wait(lsg_ctx* c, lsg_ticket ticket, int32_t* valid) { return final_wait(c, ticket, valid, true); }

int lsg_final_verify(lsg_ctx* c, const uint8_t* partials576, size_t n_partials, int32_t* valid) {
  if (!c || !valid || (n_partials && !partials576)) return LSG_ERR_INVALID_ARG;
  lsg_ticket t;
  int rc = lsg_final_submit(c, partials576, n_partials, &t);
  if (rc) return rc;
  return lsg_final_wait(c, t, valid);
}

int lsg_aggregate_pubkeys(lsg_ctx* c, const uint8_t* pks, uint32_t pk_len, size_t n, uint8_t* out96,
                          int32_t* err_code) {
  if (!c || !out96 || !err_code || (n && !pks)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  *err_code = 0;
  if (n == 0) {
    *err_code = LSG_ERR_EMPTY_AGGREGATE;
    return LSG_OK;
  }
  s->plan.clear();
  LSG_RC(util_stage_keys(s, pks, pk_len, n));
  std::vector<int32_t> off{0}, len{(int32_t)n};
  SegPlan P = slot_seg(s, 0, off, len, false, 0, 0);
  LSG_RC(upload_plan(s));
  const int np = (int)n;
  KL(s, "k_pk_decode", lsgk::pk_decode(S_(s), np, P_<uint8_t>(s->d_pk), s->pk_stride, P_<uint32_t>(s->d_pklen),
                                       P_<uint32_t>(s->d_pkp), P_<int32_t>(s->d_pkerr), P_<uint32_t>(d->d_pktab),
                                       P_<uint8_t>(d->d_pktab_ok), (uint32_t)d->pktab_n));
  LSG_RC(run_seg(s, 0, "g1_aggregate", P, P_<uint32_t>(s->d_pkp), P_<uint32_t>(s->d_agg)));
  KL(s, "k_g1p_to_bytes", lsgk::g1p_to_bytes(S_(s), 1, P_<uint32_t>(s->d_agg), P_<uint8_t>(s->d_Fb)));
  std::vector<int32_t> pkerr(n);
  LSG_HIP(s, hipMemcpyAsync(pkerr.data(), s->d_pkerr.p, 4 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(out96, s->d_Fb.p, 96, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  for (size_t k = 0; k < n; k++)
    if (pkerr[k]) {
      *err_code = pkerr[k];
      break;
    }
  return LSG_OK;
}

int lsg_aggregate_pubkeys_multi(lsg_ctx* c, const lsg_set* sets, size_t n_sets, uint8_t* out96, int32_t* err) {
  if (!c || (n_sets && (!sets || !out96 || !err)) || n_sets > 0x7fffffffull) return LSG_ERR_INVALID_ARG;
  for (size_t i = 0; i < n_sets; i++) {
    if (sets[i].n_pks && (!sets[i].pks || (sets[i].pk_len != 48 && sets[i].pk_len != 96 && sets[i].pk_len != LSG_PK_INDEX &&
                                            sets[i].pk_len != LSG_PK_BITS && sets[i].pk_len != LSG_PK_BITS_MULTI)))
      return LSG_ERR_INVALID_ARG;
    if (!multi_set_ok(sets[i])) return LSG_ERR_INVALID_ARG;
  }
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  if (n_sets == 0) return LSG_OK;
  std::vector<lsg_set> ks(n_sets);
  std::vector<const lsg_set*> sp(n_sets);
  for (size_t i = 0; i < n_sets; i++) {
    memset(&ks[i], 0, sizeof(lsg_set));
    ks[i].pks = sets[i].pks;
    ks[i].pk_len = sets[i].pk_len;
    ks[i].n_pks = sets[i].n_pks;
    sp[i] = &ks[i];
  }
  LSG_RC(stage_sets(s, sp.data(), n_sets, 0, false, nullptr, false, true));
  const size_t np = s->n_pks;
  LSG_RC(size_state(s, n_sets, np, 1, 0));
  s->plan.clear();
  const bool tree = np >= AGG_TREE_MIN_KEYS && agg_tree_on() && s->bits_sets.empty() && s->multi_sets.empty();
  s->single_keys = false;
  if (tree)
    s->agg = plan_agg_tree(s);
  else if (!s->pk_all_bits)
    s->pkagg = plan_pk_agg(s);
  s->bplan = plan_bits(s->plan, s->bits_sets);
  s->mplan = plan_multi(s->plan, s->multi_sets, s->multi_parts);
  LSG_RC(upload_plan(s));
  if (tree) {
    LSG_RC(launch_agg_tree(s, s->agg, P_<uint32_t>(s->d_agg)));
  } else if (np) {
    LSG_RC(run_pk_seg(s, s->pkagg, P_<uint32_t>(s->d_agg)));
  }
  LSG_RC(run_pk_bits(s, P_<uint32_t>(s->d_agg)));
  LSG_RC(run_pk_multi(s, P_<uint32_t>(s->d_agg)));
  LSG_RC(ensure(s, s->d_aux, 96 * n_sets));
  KL(s, "k_g1p_to_bytes", lsgk::g1p_to_bytes(S_(s), (int)n_sets, P_<uint32_t>(s->d_agg), P_<uint8_t>(s->d_aux)));
  std::vector<int32_t> pkerr(std::max(np, (size_t)1));
  if (np) LSG_HIP(s, hipMemcpyAsync(pkerr.data(), s->d_pkerr.p, 4 * np, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(out96, s->d_aux.p, 96 * n_sets, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  for (size_t i = 0; i < n_sets; i++) {
    err[i] = s->shape.pk_cnt[i] == 0 ? LSG_ERR_EMPTY_AGGREGATE : 0;
    if (!s->shape.bits_p.empty() && s->shape.bits_p[i] >= 0)
      err[i] = s->shape.bits_kerr[i] ? s->shape.bits_kerr[i] : (s->shape.bits_p[i] ? 0 : LSG_ERR_EMPTY_AGGREGATE);
    for (uint32_t q = 0; q < s->shape.pk_cnt[i] && !err[i]; q++) err[i] = pkerr[s->shape.pk_first[i] + q];
  }
  return LSG_OK;
}

int lsg_pubkey_table_set(lsg_ctx* c, size_t first, const uint8_t* pks, uint32_t pk_len, size_t n, int32_t* err) {
  if (!c || (n && !pks) || (pk_len != 48 && pk_len != 96) || first + n > 0xffffffffull) return LSG_ERR_INVALID_ARG;
  std::unique_lock<std::shared_mutex> tab(c->tab_mu);  // no package is being staged from the table
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  // a rewritten row may be a member of a registered committee, whose stored sum would then be
  // stale: every committee is unset (appends leave them alone)
  if (first < c->dev[0]->pktab_n) std::fill(c->cm_ok.begin(), c->cm_ok.end(), (uint8_t)0);
  std::vector<int32_t> pkerr;
  for (int d = 0; d < c->n_dev; d++) LSG_RC(dev_pktab_set(c->dev[d], first, pks, pk_len, n, pkerr));
  (void)hipSetDevice(c->dev[0]->device);
  if (err)
    for (size_t k = 0; k < n; k++) err[k] = pkerr[k];
  return LSG_OK;
}

// The message cache: per device an arena of `capacity` affine H(m) rows in the
// lane layout with one infinity flag each, and the host policy's key store (lsg_msg_cache.hpp).
// Like a pubkey-table rewrite it takes the staging lock exclusively and drains the devices;
// what launches still unwaited pinned or wrote belongs to the epoch that ends here.
static int msg_cache_reset(lsg_ctx* c, size_t capacity, bool realloc) {
  std::unique_lock<std::shared_mutex> tab(c->tab_mu);  // no package is being staged
  LSG_ENTER(c);
  int rc = LSG_OK;
  for (int i = 0; i < c->n_dev && !rc; i++) {
    Dev* d = c->dev[i];
    LSG_HIPC(c, hipSetDevice(d->device));
    LSG_HIPC(c, hipDeviceSynchronize());
    if (!realloc) {
      d->mc.clear();
      continue;
    }
    d->mc.resize(0);
    free_dev(d->d_mc_rows);
    free_dev(d->d_mc_inf);
    if (!capacity) continue;
    hipError_t e = hipMalloc(&d->d_mc_rows.p, 4 * W_G2A * capacity);
    if (e == hipSuccess) {
      g_allocs++;
      d->d_mc_rows.cap = 4 * W_G2A * capacity;
      e = hipMalloc(&d->d_mc_inf.p, capacity);
    }
    if (e == hipSuccess) {
      g_allocs++;
      d->d_mc_inf.cap = capacity;
      e = hipMemset(d->d_mc_inf.p, 0, capacity);
    }
    if (e != hipSuccess) {
      rc = fail_c(c, "hipMalloc", e);
      break;
    }
    d->mc.resize(capacity);
  }
  if (rc)  // no half-enabled context: the cache is off on every device
    for (int i = 0; i < c->n_dev; i++) {
      (void)hipSetDevice(c->dev[i]->device);
      c->dev[i]->mc.resize(0);
      free_dev(c->dev[i]->d_mc_rows);
      free_dev(c->dev[i]->d_mc_inf);
    }
  (void)hipSetDevice(c->dev[0]->device);
  return rc;
}

int lsg_msg_cache_set(lsg_ctx* c, size_t capacity) {
  if (!c || capacity >= LSG_MC_ROW) return LSG_ERR_INVALID_ARG;
  return msg_cache_reset(c, capacity, true);
}

int lsg_msg_cache_clear(lsg_ctx* c) {
  if (!c) return LSG_ERR_INVALID_ARG;
  return msg_cache_reset(c, 0, false);
}

int lsg_msg_cache_get_stats(lsg_ctx* c, lsg_msg_cache_stats* out) {
  if (!c || !out) return LSG_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  memset(out, 0, sizeof(*out));
  for (int i = 0; i < c->n_dev; i++) {
    const MsgCacheStats t = c->dev[i]->mc.stats();
    out->lookups += t.lookups;
    out->hits += t.hits;
    out->pending += t.pending;
    out->inserts += t.inserts;
    out->evictions += t.evictions;
    out->bypassed += t.bypassed;
    out->full += t.full;
    out->entries += t.entries;
    out->capacity += t.capacity;
  }
  return LSG_OK;
}

int lsg_committees_set(lsg_ctx* c, uint32_t first_id, const uint32_t* indices, const uint32_t* offsets, size_t n,
                       int32_t* err) {
  if (!c || (n && !offsets) || first_id > COMMITTEE_MAX_ID || n > COMMITTEE_MAX_ID - first_id) return LSG_ERR_INVALID_ARG;
  if (n == 0) return LSG_OK;
  if (offsets[0] != 0) return LSG_ERR_INVALID_ARG;
  for (size_t k = 0; k < n; k++)
    if (offsets[k + 1] < offsets[k] || offsets[k + 1] - offsets[k] > COMMITTEE_MAX_LEN) return LSG_ERR_INVALID_ARG;
  const size_t total = offsets[n];
  if ((total && !indices) || total > 0x7fffffffull) return LSG_ERR_INVALID_ARG;
  std::unique_lock<std::shared_mutex> tab(c->tab_mu);  // no package is being staged from the committees
  LSG_ENTER(c);
  // host rows: the new committees appended; the rows they replace become dead words
  const size_t ids = std::max(c->cm_ok.size(), (size_t)first_id + n);
  c->cm_len.resize(ids, 0);
  c->cm_off.resize(ids, 0);
  c->cm_ok.resize(ids, 0);
  for (size_t k = 0; k < n; k++) {
    c->cm_dead += c->cm_len[first_id + k];
    c->cm_len[first_id + k] = 0;
    c->cm_ok[first_id + k] = 0;
  }
  if (c->cm_dead > c->cm_rows.size() / 2 + 65536) {  // compact: the live committees in id order
    std::vector<uint32_t> rows;
    rows.reserve(c->cm_rows.size() - c->cm_dead + total);
    for (size_t id = 0; id < ids; id++) {
      const uint32_t o = c->cm_off[id];
      c->cm_off[id] = (uint32_t)rows.size();
      if (c->cm_ok[id]) rows.insert(rows.end(), c->cm_rows.begin() + o, c->cm_rows.begin() + o + c->cm_len[id]);
      else c->cm_len[id] = 0;
    }
    c->cm_rows.swap(rows);
    c->cm_dead = 0;
  }
  const size_t base = c->cm_rows.size();
  if (base + total > 0xffffffffull) {
    c->err = "lsg_committees_set: more than 2^32 committee members registered";
    return LSG_ERR_INVALID_ARG;
  }
  if (total) c->cm_rows.insert(c->cm_rows.end(), indices, indices + total);
  // the sums: the aggregation over index keys, one set per committee, on every device
  std::vector<lsg_set> ks(n);
  std::vector<const lsg_set*> sp(n);
  for (size_t k = 0; k < n; k++) {
    memset(&ks[k], 0, sizeof(lsg_set));
    ks[k].pks = (const uint8_t*)(indices + offsets[k]);
    ks[k].pk_len = LSG_PK_INDEX;
    ks[k].n_pks = offsets[k + 1] - offsets[k];
    sp[k] = &ks[k];
  }
  std::vector<int32_t> cerr(n, 0), pkerr(std::max(total, (size_t)1));
  for (int di = 0; di < c->n_dev; di++) {
    Dev* d = c->dev[di];
    Slot* s = &d->util;
    LSG_HIPC(c, hipSetDevice(d->device));
    // packages in flight read the rows and sums: drain the device before they move or change
    LSG_HIPC(c, hipDeviceSynchronize());
    timer_reset(s);
    // grow (copying what is there), then rewrite the whole index arena when it was compacted
    auto grow = [&](DevBuf& b, size_t bytes) -> int {
      if (b.cap >= bytes) return LSG_OK;
      DevBuf nb;
      const size_t cap = std::max(bytes + bytes / 2, (size_t)65536);
      LSG_HIPC(c, hipMalloc(&nb.p, cap));
      g_allocs++;
      trace_alloc("device", cap);
      nb.cap = cap;
      if (b.p) LSG_HIPC(c, hipMemcpy(nb.p, b.p, b.cap, hipMemcpyDeviceToDevice));
      free_dev(b);
      b = nb;
      return LSG_OK;
    };
    LSG_RC(grow(d->d_cm_idx, 4 * c->cm_rows.size()));
    LSG_RC(grow(d->d_cm_off, 4 * ids));
    LSG_RC(grow(d->d_cm_sum, 4 * W_G1P * ids));
    LSG_RC(stage_sets(s, sp.data(), n, 0, false));
    LSG_RC(size_state(s, n, 0, 1, 0));  // (no projective copy of the keys: the fold fetches them)
    LSG_RC(ensure(s, s->d_pkerr, 4 * total));
    s->plan.clear();
    s->single_keys = false;
    s->pkagg = plan_pk_agg(s);
    LSG_RC(upload_plan(s));
    LSG_RC(run_pk_seg(s, s->pkagg, P_<uint32_t>(s->d_agg)));
    if (total) LSG_HIP(s, hipMemcpyAsync(pkerr.data(), s->d_pkerr.p, 4 * total, hipMemcpyDeviceToHost, s->st[0]));
    LSG_HIP(s, hipMemcpyAsync(P_<uint32_t>(d->d_cm_sum) + W_G1P * (size_t)first_id, s->d_agg.p, 4 * W_G1P * n,
                              hipMemcpyDeviceToDevice, s->st[0]));
    LSG_HIP(s, hipStreamSynchronize(s->st[0]));
    keep_times(s);
    for (size_t k = 0; k < n; k++) {
      int32_t e = offsets[k + 1] == offsets[k] ? LSG_ERR_EMPTY_AGGREGATE : 0;
      for (uint32_t q = offsets[k]; q < offsets[k + 1] && !e; q++) e = pkerr[q];
      if (e && !cerr[k]) cerr[k] = e;
    }
  }
  for (size_t k = 0; k < n; k++) {
    c->cm_off[first_id + k] = (uint32_t)(base + offsets[k]);
    if (cerr[k]) {  // stays unset: its rows are dead at once
      c->cm_dead += offsets[k + 1] - offsets[k];
      continue;
    }
    c->cm_len[first_id + k] = offsets[k + 1] - offsets[k];
    c->cm_ok[first_id + k] = 1;
  }
  for (int di = 0; di < c->n_dev; di++) {
    Dev* d = c->dev[di];
    LSG_HIPC(c, hipSetDevice(d->device));
    // (after a compaction every offset moved: the whole arena and offset list go up again)
    LSG_HIPC(c, hipMemcpy(d->d_cm_idx.p, c->cm_rows.data(), 4 * c->cm_rows.size(), hipMemcpyHostToDevice));
    LSG_HIPC(c, hipMemcpy(d->d_cm_off.p, c->cm_off.data(), 4 * ids, hipMemcpyHostToDevice));
  }
  (void)hipSetDevice(c->dev[0]->device);
  if (err)
    for (size_t k = 0; k < n; k++) err[k] = cerr[k];
  return LSG_OK;
}

int lsg_committees_clear(lsg_ctx* c, uint32_t first_id, size_t n) {
  if (!c || first_id > COMMITTEE_MAX_ID || n > COMMITTEE_MAX_ID - first_id) return LSG_ERR_INVALID_ARG;
  std::unique_lock<std::shared_mutex> tab(c->tab_mu);
  std::lock_guard<std::mutex> lk(c->mu);
  for (size_t id = first_id; id < (size_t)first_id + n && id < c->cm_ok.size(); id++) {
    c->cm_dead += c->cm_len[id];
    c->cm_len[id] = 0;
    c->cm_ok[id] = 0;
  }
  return LSG_OK;
}

int lsg_committee_count(lsg_ctx* c, size_t* n) {
  if (!c || !n) return LSG_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  size_t hi = c->cm_ok.size();
  while (hi && !c->cm_ok[hi - 1]) hi--;
  *n = hi;
  return LSG_OK;
}

int lsg_pubkey_table_size(lsg_ctx* c, size_t* n) {
  if (!c || !n) return LSG_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  *n = c->dev[0]->pktab_n;
  return LSG_OK;
}

int lsg_pubkey_validate(lsg_ctx* c, const uint8_t* pks, uint32_t pk_len, size_t n, uint8_t* out96, int32_t* err) {
  if (!c || !err || (n && !pks) || (pk_len != 48 && pk_len != 96) || n > 0x7fffffffull) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  LSG_RC(util_stage_keys(s, pks, pk_len, n));
  LSG_RC(ensure(s, s->d_ub, 96 * n));
  KL(s, "k_pk_validate", lsgk::pk_validate(S_(s), (int)n, P_<uint8_t>(s->d_pk), pk_len, P_<uint32_t>(s->d_pkp),
                                           P_<int32_t>(s->d_pkerr)));
  LSG_HIP(s, hipMemcpyAsync(err, s->d_pkerr.p, 4 * n, hipMemcpyDeviceToHost, s->st[0]));
  if (out96) {
    KL(s, "k_g1p_to_bytes", lsgk::g1p_to_bytes(S_(s), (int)n, P_<uint32_t>(s->d_pkp), P_<uint8_t>(s->d_ub)));
    LSG_HIP(s, hipMemcpyAsync(out96, s->d_ub.p, 96 * n, hipMemcpyDeviceToHost, s->st[0]));
  }
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

int lsg_hash_to_g2(lsg_ctx* c, const uint8_t* msgs, uint32_t msg_len, size_t n, const uint8_t* dst,
                   uint32_t dst_len, uint8_t* out192) {
  if (!c || !out192 || (n && msg_len && !msgs) || dst_len > 255 || (dst_len && !dst) || msg_marked(msg_len))
    return LSG_ERR_INVALID_ARG;  // (these are plain messages: LSG_MSG_OBJECT is a set form)
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  LSG_RC(util_hash(s, msgs, msg_len, n, dst, dst_len));
  LSG_RC(ensure(s, s->d_aux, 192 * n));
  const int nn = (int)n;
  KL(s, "k_g2a_to_bytes",
     lsgk::g2a_to_bytes(S_(s), nn, P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf), P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out192, s->d_aux.p, 192 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

// Signature.fromBytes(sig, affine, validate) for n signatures (subgroup check when validate)
static int sig_decode_impl(lsg_ctx* c, const uint8_t* sigs, uint32_t sig_len, size_t n, bool validate, Slot** out) {
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  *out = s;
  std::vector<lsg_set> sets(n);
  std::vector<const lsg_set*> sp(n);
  for (size_t i = 0; i < n; i++) {
    memset(&sets[i], 0, sizeof(lsg_set));
    sets[i].sig = sigs + (size_t)sig_len * i;
    sets[i].sig_len = sig_len;
    sp[i] = &sets[i];
  }
  LSG_RC(stage_sets(s, sp.data(), n, 0, false));
  LSG_RC(size_state(s, n, 0, 1, 0));
  const int nn = (int)n;
  const lsgk::PowLanes pw = pow_lanes(s->d_pwsig, n, lsgk::POW_SIG_STATE);
  KL(s, "k_sig_decode", lsgk::sig_decode(S_(s), nn, P_<uint8_t>(s->d_sig), P_<uint32_t>(s->d_siglen),
                                         P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf), P_<int32_t>(s->d_seterr), pw));
  KL_POW(s, pw, nn);
  if (validate) LSG_RC(launch_sig_subgroup(s, nn));
  return LSG_OK;
}

int lsg_sig_decode(lsg_ctx* c, const uint8_t* sigs, uint32_t sig_len, size_t n, uint8_t* out192, int32_t* err) {
  if (!c || !out192 || !err || (n && !sigs)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  timer_reset(&c->dev[0]->util);
  if (n == 0) return LSG_OK;
  Slot* s;
  LSG_RC(sig_decode_impl(c, sigs, sig_len, n, true, &s));
  LSG_RC(ensure(s, s->d_aux, 192 * n));
  KL(s, "k_g2a_to_bytes", lsgk::g2a_to_bytes(S_(s), (int)n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                             P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out192, s->d_aux.p, 192 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(err, s->d_seterr.p, 4 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

// G2 signature aggregation for the op pools: n_groups Signature.aggregate
// calls in one pass -- decode without the subgroup check (signatureFromBytesNoCheck,
// opPools/utils.ts:32-34), one segmented reduction, one compression per group
int lsg_aggregate_signatures(lsg_ctx* c, const uint8_t* sigs, uint32_t sig_len, const uint32_t* offsets,
                             size_t n_groups, uint8_t* out96, int32_t* err) {
  if (!c || !offsets || (n_groups && (!out96 || !err)) || offsets[0] != 0 || n_groups > 0x7fffffffull)
    return LSG_ERR_INVALID_ARG;
  for (size_t g = 0; g < n_groups; g++)
    if (offsets[g + 1] < offsets[g]) return LSG_ERR_INVALID_ARG;
  const size_t n = offsets[n_groups];
  if (n && !sigs) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  timer_reset(&c->dev[0]->util);
  for (size_t g = 0; g < n_groups; g++) {
    err[g] = offsets[g + 1] == offsets[g] ? LSG_ERR_EMPTY_AGGREGATE : 0;
    memset(out96 + 96 * g, 0, 96);
  }
  if (n == 0) return LSG_OK;
  Slot* s;
  LSG_RC(sig_decode_impl(c, sigs, sig_len, n, false, &s));
  LSG_RC(size_state(s, n, 0, n_groups, 0));
  s->plan.clear();
  std::vector<int32_t> off(n_groups), len(n_groups);
  for (size_t g = 0; g < n_groups; g++) {
    off[g] = (int32_t)offsets[g];
    len[g] = (int32_t)(offsets[g + 1] - offsets[g]);
  }
  SegPlan P = slot_seg(s, 1, off, len, false, 0, 0);
  LSG_RC(upload_plan(s));
  LSG_RC(ensure(s, s->d_aux, 96 * n_groups));
  const int nn = (int)n;
  KL(s, "k_sig_prep", lsgk::sig_prep(S_(s), nn, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                     P_<int32_t>(s->d_seterr), nullptr, nullptr, nullptr, P_<uint32_t>(s->d_rs)));
  LSG_RC(run_seg(s, 1, "g2_aggregate", P, P_<uint32_t>(s->d_rs), P_<uint32_t>(s->d_S)));
  KL(s, "k_g2p_compress",
     lsgk::g2p_compress(S_(s), (int)n_groups, P_<uint32_t>(s->d_S), P_<uint8_t>(s->d_aux)));
  std::vector<int32_t> serr(n);
  std::vector<uint8_t> blob(96 * n_groups);
  LSG_HIP(s, hipMemcpyAsync(serr.data(), s->d_seterr.p, 4 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(blob.data(), s->d_aux.p, 96 * n_groups, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  // Signature.aggregate throws on the first signature that fails to deserialize
  for (size_t g = 0; g < n_groups; g++) {
    if (offsets[g + 1] == offsets[g]) continue;
    for (uint32_t i = offsets[g]; i < offsets[g + 1] && !err[g]; i++) err[g] = serr[i];
    if (!err[g]) memcpy(out96 + 96 * g, blob.data() + 96 * g, 96);
  }
  return LSG_OK;
}

// SSZ signing roots; kind 0: object roots given, 1: AttestationData bytes,
// 2: DepositMessage bytes, 3: any kind of LSG_MSG_OBJECT by its serialized length obj_len
// (the dispatcher of lsg_ssz.hpp that k_msg_roots runs)
static int signing_roots(lsg_ctx* c, int kind, const uint8_t* objs, size_t n, const uint8_t* domain, uint32_t dstride,
                         uint8_t* out32, uint32_t obj_len = 0) {
  const size_t ob = kind == 3 ? obj_len : (kind == 2 ? 88 : (kind ? 128 : 32));
  if (kind == 3 && msg_object_kind(LSG_MSG_OBJECT | (obj_len + 32)) != obj_len) return LSG_ERR_INVALID_ARG;
  if (!c || !domain || (dstride != 0 && dstride != 32) || (n && (!objs || !out32)) || n > 0x7fffffffull)
    return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  const size_t nd = dstride ? n : 1;
  LSG_RC(ensure(s, s->d_aux, ob * n + 32 * nd));
  LSG_RC(ensure(s, s->d_Fb, 32 * n));
  uint8_t* d_obj = P_<uint8_t>(s->d_aux);
  uint8_t* d_dom = d_obj + ob * n;
  LSG_HIP(s, hipMemcpyAsync(d_obj, objs, ob * n, hipMemcpyHostToDevice, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(d_dom, domain, 32 * nd, hipMemcpyHostToDevice, s->st[0]));
  const int nn = (int)n;
  if (kind == 3)
    KL(s, "k_object_signing_root",
       lsgk::object_signing_root(S_(s), nn, d_obj, obj_len, d_dom, dstride, P_<uint8_t>(s->d_Fb)));
  else if (kind == 2)
    KL(s, "k_deposit_signing_root",
       lsgk::deposit_signing_root(S_(s), nn, d_obj, 88, d_dom, dstride, P_<uint8_t>(s->d_Fb)));
  else if (kind)
    KL(s, "k_attestation_signing_root",
       lsgk::attestation_signing_root(S_(s), nn, d_obj, d_dom, dstride, P_<uint8_t>(s->d_Fb)));
  else
    KL(s, "k_signing_root", lsgk::signing_root(S_(s), nn, d_obj, d_dom, dstride, P_<uint8_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out32, s->d_Fb.p, 32 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

int lsg_signing_roots(lsg_ctx* c, const uint8_t* roots32, size_t n, const uint8_t* domain32, uint32_t domain_stride,
                      uint8_t* out32) {
  return signing_roots(c, 0, roots32, n, domain32, domain_stride, out32);
}

int lsg_attestation_signing_roots(lsg_ctx* c, const uint8_t* data128, size_t n, const uint8_t* domain32,
                                  uint32_t domain_stride, uint8_t* out32) {
  return signing_roots(c, 1, data128, n, domain32, domain_stride, out32);
}

int lsg_deposit_signing_roots(lsg_ctx* c, const uint8_t* msgs88, size_t n, const uint8_t* domain32,
                              uint32_t domain_stride, uint8_t* out32) {
  return signing_roots(c, 2, msgs88, n, domain32, domain_stride, out32);
}

int lsg_object_signing_roots(lsg_ctx* c, const uint8_t* objs, uint32_t obj_len, size_t n, const uint8_t* domain32,
                             uint32_t domain_stride, uint8_t* out32) {
  return signing_roots(c, 3, objs, n, domain32, domain_stride, out32, obj_len);
}

// The variable-size kinds through k_msg_roots_var, the kernel a package runs for tagged sets:
// the payloads object || domain are laid out back to back as a package's messages are, with
// their offsets and tagged length words; the roots come back in a list of their own.
int lsg_object_signing_roots_var(lsg_ctx* c, uint32_t kind, const uint8_t* objs, const uint32_t* offsets, size_t n,
                                 const uint8_t* domain, uint32_t dstride, uint8_t* out32) {
  if (!c || !domain || (dstride != 0 && dstride != 32) || (n && (!objs || !offsets || !out32)) || n > 0x7fffffffull ||
      (kind != LSG_MSG_KIND_AGG_PROOF && kind != LSG_MSG_KIND_AGG_PROOF_ELECTRA))
    return LSG_ERR_INVALID_ARG;
  if (n && offsets[0] != 0) return LSG_ERR_INVALID_ARG;
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    if (offsets[i + 1] < offsets[i] || !msg_var_ok(kind, objs + offsets[i], offsets[i + 1] - offsets[i]))
      return LSG_ERR_INVALID_ARG;
    total += (uint64_t)(offsets[i + 1] - offsets[i]) + 32;
  }
  if (total > 0xffffffffull) return LSG_ERR_INVALID_ARG;  // (staged offsets are 32-bit)
  LSG_ENTER(c);
  Dev* d = c->dev[0];
  Slot* s = &d->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  // host image: payloads (8-aligned size), then the offsets, then the length words
  const size_t pay = ((size_t)total + 7) & ~(size_t)7;
  std::vector<uint8_t> img(pay + 8 * n);
  uint32_t* off = (uint32_t*)(img.data() + pay);
  uint32_t* len = off + n;
  size_t at = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t ol = offsets[i + 1] - offsets[i];
    off[i] = (uint32_t)at;
    len[i] = LSG_MSG_OBJECT | (kind << LSG_MSG_KIND_SHIFT) | (ol + 32);
    memcpy(img.data() + at, objs + offsets[i], ol);
    memcpy(img.data() + at + ol, domain + (size_t)dstride * i, 32);
    at += (size_t)ol + 32;
  }
  LSG_RC(ensure(s, s->d_aux, img.size()));
  LSG_RC(ensure(s, s->d_Fb, 32 * n));
  uint8_t* d_img = P_<uint8_t>(s->d_aux);
  LSG_HIP(s, hipMemcpyAsync(d_img, img.data(), img.size(), hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_msg_roots_var", lsgk::msg_roots_var(S_(s), (int)n, d_img, (const uint32_t*)(d_img + pay),
                                               (uint32_t*)(d_img + pay) + n, P_<uint8_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out32, s->d_Fb.p, 32 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

// processDeposit.ts:47-66 for n deposits: signing roots on the device, then one single-set
// batchable LSG_JOB_VALIDATE_KEYS job per deposit through the package machinery
int lsg_verify_deposits(lsg_ctx* c, const uint8_t* data184, size_t n, const uint8_t* domain32, uint64_t seed,
                        uint8_t* valid, int32_t* err) {
  if (!c || !domain32 || (n && (!data184 || !valid || !err)) || n > 0x7fffffffull) return LSG_ERR_INVALID_ARG;
  if (n == 0) return LSG_OK;
  memset(valid, 0, n);
  memset(err, 0, 4 * n);
  std::lock_guard<std::mutex> dep(c->dep_mu);
  Dev* d = c->dev[0];
  const bool resident = c->n_dev == 1;  // the roots stay on the device as the packages' messages
  std::vector<uint8_t> host_roots(resident ? 0 : 32 * n);
  {
    LSG_ENTER(c);
    Slot* s = &d->util;
    timer_reset(s);
    LSG_RC(ensure(s, d->d_dep_in, 184 * n + 32));
    LSG_RC(ensure(s, d->d_dep_roots, 32 * n));
    uint8_t* d_in = P_<uint8_t>(d->d_dep_in);
    LSG_HIP(s, hipMemcpyAsync(d_in, data184, 184 * n, hipMemcpyHostToDevice, s->st[0]));
    LSG_HIP(s, hipMemcpyAsync(d_in + 184 * n, domain32, 32, hipMemcpyHostToDevice, s->st[0]));
    KL(s, "k_deposit_signing_root",
       lsgk::deposit_signing_root(S_(s), (int)n, d_in, 184, d_in + 184 * n, 0, P_<uint8_t>(d->d_dep_roots)));
    if (!resident)  // a multi-device context stages each device's share from the host
      LSG_HIP(s, hipMemcpyAsync(host_roots.data(), d->d_dep_roots.p, 32 * n, hipMemcpyDeviceToHost, s->st[0]));
    LSG_HIP(s, hipStreamSynchronize(s->st[0]));
    keep_times(s);
  }
  static const uint8_t zero32[32] = {0};
  std::vector<lsg_set> sets(n);
  std::vector<lsg_job> jobs(n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* dd = data184 + 184 * i;
    sets[i].pks = dd;
    sets[i].pk_len = 48;
    sets[i].n_pks = 1;
    sets[i].msg = resident ? zero32 : host_roots.data() + 32 * i;
    sets[i].msg_len = 32;
    sets[i].sig = dd + 88;
    sets[i].sig_len = 96;
    jobs[i].sets = &sets[i];
    jobs[i].n_sets = 1;
    jobs[i].flags = LSG_JOB_BATCHABLE | LSG_JOB_VALIDATE_KEYS;
  }
  // packages of at most DEPOSIT_PKG deposits, at most DEPOSIT_INFLIGHT of them outstanding
  // (enough to keep the device full; the other slots stay free for the host's own packages
  // and its priority jobs), waited on in order
  constexpr size_t DEPOSIT_PKG = 8192, DEPOSIT_INFLIGHT = 4;
  struct Out {
    lsg_ticket t;
    size_t first, count;
  };
  std::vector<Out> out;  // outstanding, oldest first
  std::vector<lsg_job_result> res(std::min(n, DEPOSIT_PKG));
  int rc = LSG_OK;
  auto wait_oldest = [&]() {
    const Out o = out.front();
    out.erase(out.begin());
    const int w = lsg_wait_jobs(c, o.t, res.data(), nullptr);
    if (w) return w;
    for (size_t k = 0; k < o.count; k++) {
      valid[o.first + k] = res[k].status == LSG_VALID ? 1 : 0;
      err[o.first + k] = res[k].status == LSG_ERROR ? res[k].err_code : 0;
    }
    return (int)LSG_OK;
  };
  size_t pkg = 0;
  for (size_t o = 0; o < n && !rc; pkg++) {
    const size_t cnt = std::min(DEPOSIT_PKG, n - o);
    lsg_ticket t = 0;
    if (out.size() >= DEPOSIT_INFLIGHT) {
      rc = wait_oldest();
      pkg--;
      continue;
    }
    {
      CtxLock lk(c->mu);
      const hipError_t he = hipSetDevice(d->device);
      if (he != hipSuccess)  // (no early return: the tickets already out are drained below)
        rc = fail_c(c, "hipSetDevice", he);
      else
        rc = submit_pkg(c, lk, jobs.data() + o, cnt, seed ? seed + 0x9e3779b97f4a7c15ull * pkg : 0, &t, true,
                        resident ? P_<uint8_t>(d->d_dep_roots) + 32 * o : nullptr);
    }
    if (rc == LSG_ERR_BUSY && !out.empty()) {  // every slot is taken: free this call's oldest
      rc = wait_oldest();
      pkg--;
      continue;
    }
    if (rc) break;
    out.push_back({t, o, cnt});
    o += cnt;
  }
  while (!out.empty()) {  // (after an error too: no ticket of this call stays outstanding)
    const int w = wait_oldest();
    if (!rc) rc = w;
  }
  return rc;
}

int lsg_sign(lsg_ctx* c, const uint8_t* sks32, const uint8_t* msgs, uint32_t msg_len, size_t n, uint8_t* out96) {
  if (!c || !out96 || (n && (!sks32 || !msgs)) || msg_marked(msg_len)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  LSG_RC(util_hash(s, msgs, msg_len, n, DST_POP, DST_POP_LEN));
  LSG_RC(ensure(s, s->d_aux, 96 * n));
  LSG_RC(ensure(s, s->d_Fb, 32 * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_Fb.p, sks32, 32 * n, hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_sign", lsgk::sign(S_(s), (int)n, P_<uint8_t>(s->d_Fb), P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out96, s->d_aux.p, 96 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}

int lsg_sk_to_pk(lsg_ctx* c, const uint8_t* sks32, size_t n, uint8_t* out96) {
  if (!c || !out96 || (n && !sks32)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  if (n == 0) return LSG_OK;
  LSG_RC(ensure(s, s->d_aux, 96 * n));
  LSG_RC(ensure(s, s->d_Fb, 32 * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_Fb.p, sks32, 32 * n, hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_sk_to_pk", lsgk::sk_to_pk(S_(s), (int)n, P_<uint8_t>(s->d_Fb), P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out96, s->d_aux.p, 96 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}

int lsg_check_fp2_mul(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) {
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * 4 * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * 2 * W_FP * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * 4 * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_check_fp2_mul", lsgk::check_fp2_mul(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * 2 * W_FP * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}

// the squaring hooks: E elements per item in, E out (E = 1: fp_sqr, E = 2: fp2_sqr)
static int check_sqr(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out, int E) {
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  const size_t bytes = 4 * (size_t)E * W_FP * n;
  LSG_RC(ensure(s, s->d_aux, bytes));
  LSG_RC(ensure(s, s->d_Fb, bytes));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, bytes, hipMemcpyHostToDevice, s->st[0]));
  if (E == 1)
    KL(s, "k_check_fp_sqr", lsgk::check_fp_sqr(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  else
    KL(s, "k_check_fp2_sqr", lsgk::check_fp2_sqr(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, bytes, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}
int lsg_check_fp_sqr(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) { return check_sqr(c, in, n, out, 1); }
int lsg_check_fp2_sqr(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) { return check_sqr(c, in, n, out, 2); }

// the lazy-sum hook (k_check_sums): 12 elements per item in, 42 out
int lsg_check_sums(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) {
  constexpr size_t EIN = 12, EOUT = 42;
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP * EOUT)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * EIN * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * EOUT * W_FP * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * EIN * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_check_sums", lsgk::check_sums(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * EOUT * W_FP * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}

// the component-per-lane Fp2 hooks (k_check_fp2_lanes, k_check_g2_lanes, k_check_mf_lanes): EIN elements per
// item in, EOUT out
static int check_lanes(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out, bool g2, bool mf = false) {
  const size_t EIN = g2 ? lsgk::CHECK_G2L_IN : lsgk::CHECK_LANES_IN, EOUT = g2 ? lsgk::CHECK_G2L_OUT : lsgk::CHECK_LANES_OUT;
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP * EOUT)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * EIN * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * EOUT * W_FP * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * EIN * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  if (g2)
    KL(s, "k_check_g2_lanes", lsgk::check_g2_lanes(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  else if (mf)
    KL(s, "k_check_mf_lanes", lsgk::check_mf_lanes(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  else
    KL(s, "k_check_fp2_lanes", lsgk::check_fp2_lanes(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * EOUT * W_FP * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}
int lsg_check_fp2_lanes(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) { return check_lanes(c, in, n, out, false); }
int lsg_check_g2_lanes(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) { return check_lanes(c, in, n, out, true); }
int lsg_check_mf_lanes(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) {
  return check_lanes(c, in, n, out, false, true);
}

// the fixed-exponent power hooks (k_fp_pow_lanes, k_check_pow_pair): n elements in, n out
static int check_pow(lsg_ctx* c, int32_t id, const uint32_t* in, size_t n, uint32_t* out, bool lanes) {
  if (!c || id < 0 || id > 2 || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * W_FP * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  if (lanes)
    KL(s, "k_fp_pow_lanes", lsgk::fp_pow_lanes(S_(s), (int)n, id, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  else
    KL(s, "k_check_pow_pair", lsgk::check_pow_pair(S_(s), (int)n, id, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * W_FP * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}
int lsg_check_pow_lanes(lsg_ctx* c, int32_t id, const uint32_t* in, size_t n, uint32_t* out) {
  return check_pow(c, id, in, n, out, true);
}
int lsg_check_pow_pair(lsg_ctx* c, int32_t id, const uint32_t* in, size_t n, uint32_t* out) {
  return check_pow(c, id, in, n, out, false);
}

// the bucket-pass hook (k_msm_bucket_seg and its pair-form twin; mode 2: k_sig_proj + k_seg_reduce<1>)
int lsg_check_msm_buckets(lsg_ctx* c, int32_t mode, const uint8_t* sigs96, size_t n, const int32_t* err,
                          const uint8_t* inf, const uint8_t* pinf, const int32_t* idx, size_t n_idx,
                          const int32_t* chunks, size_t n_chunks, int32_t ips_log2, const int32_t* chunks2,
                          size_t n_chunks2, int32_t ips_log2_2, size_t n_tmp, size_t n_out, uint8_t* out96) {
  const size_t lim = (size_t)1 << 20;
  if (!c || mode < 0 || mode > 2 || !sigs96 || !err || !inf || !pinf || !chunks || !out96 || (n_idx && !idx) ||
      (n_chunks2 && !chunks2) || n == 0 || n > lim || n_idx > lim || n_chunks == 0 || n_chunks > lim || n_chunks2 > lim ||
      n_tmp > lim || n_out == 0 || n_out > lim || ips_log2 < 0 || ips_log2 > 5 || ips_log2_2 < 0 || ips_log2_2 > 5)
    return LSG_ERR_INVALID_ARG;
  // every index the kernels follow is checked here: list entries name a point, a chunk lies
  // inside its list, every tmp slot and every output is written exactly once
  for (size_t k = 0; k < n_idx; k++)
    if (idx[k] < 0 || (size_t)idx[k] >= n) return LSG_ERR_INVALID_ARG;
  std::vector<uint8_t> tmp_set(n_tmp, 0), out_set(n_out, 0);
  auto mark = [&](int32_t out, bool tmp_ok) {
    std::vector<uint8_t>& v = out >= 0 ? out_set : tmp_set;
    const size_t o = out >= 0 ? (size_t)out : (size_t)(-(int64_t)out - 1);
    if ((out < 0 && !tmp_ok) || o >= v.size() || v[o]) return false;
    v[o] = 1;
    return true;
  };
  for (size_t k = 0; k < n_chunks; k++) {
    const int32_t off = chunks[3 * k], len = chunks[3 * k + 1];
    if (off < 0 || len < 0 || (size_t)off + (size_t)len > n_idx || !mark(chunks[3 * k + 2], true)) return LSG_ERR_INVALID_ARG;
  }
  for (size_t k = 0; k < n_chunks2; k++) {
    const int32_t off = chunks2[3 * k], len = chunks2[3 * k + 1];
    if (off < 0 || len < 0 || (size_t)off + (size_t)len > n_tmp || !mark(chunks2[3 * k + 2], false)) return LSG_ERR_INVALID_ARG;
  }
  for (uint8_t v : tmp_set)
    if (!v) return LSG_ERR_INVALID_ARG;
  for (uint8_t v : out_set)
    if (!v) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  timer_reset(&c->dev[0]->util);
  Slot* s;
  LSG_RC(sig_decode_impl(c, sigs96, 96, n, false, &s));
  LSG_HIP(s, hipMemcpyAsync(s->d_seterr.p, err, 4 * n, hipMemcpyHostToDevice, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(s->d_siginf.p, inf, n, hipMemcpyHostToDevice, s->st[0]));
  LSG_HIP(s, hipMemcpyAsync(s->d_pinf.p, pinf, n, hipMemcpyHostToDevice, s->st[0]));
  s->plan.assign(idx, idx + n_idx);
  const size_t c1 = s->plan.size();
  s->plan.insert(s->plan.end(), chunks, chunks + 3 * n_chunks);
  const size_t c2 = s->plan.size();
  if (n_chunks2) s->plan.insert(s->plan.end(), chunks2, chunks2 + 3 * n_chunks2);
  LSG_RC(upload_plan(s));
  LSG_RC(ensure(s, s->d_bkt, 4 * W_G2P * n_out));
  LSG_RC(ensure(s, s->seg_tmp[1][0], 4 * W_G2P * std::max(n_tmp, (size_t)1)));
  LSG_RC(ensure(s, s->d_aux, 96 * n_out));
  uint32_t* dst = P_<uint32_t>(s->d_bkt);
  uint32_t* tmp = P_<uint32_t>(s->seg_tmp[1][0]);
  if (mode == 2) {
    KL(s, "k_sig_prep", lsgk::sig_prep(S_(s), (int)n, P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                       P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), nullptr, nullptr,
                                       P_<uint32_t>(s->d_rs)));
    KL(s, "msm_buckets", lsgk::seg_reduce(S_(s), 1, (int)n_chunks, ips_log2, PL(s, c1), PL(s, 0), P_<uint32_t>(s->d_rs),
                                          dst, tmp));
  } else {
    KL(s, "msm_buckets", lsgk::msm_bucket_seg(S_(s), (int)n_chunks, ips_log2, PL(s, c1), PL(s, 0),
                                              P_<uint32_t>(s->d_sigaff), P_<uint8_t>(s->d_siginf),
                                              P_<int32_t>(s->d_seterr), P_<uint8_t>(s->d_pinf), dst, tmp, mode == 1));
  }
  if (n_chunks2)
    KL(s, "msm_buckets", lsgk::seg_reduce(S_(s), 1, (int)n_chunks2, ips_log2_2, PL(s, c2), nullptr, tmp, dst, nullptr));
  KL(s, "k_g2p_compress", lsgk::g2p_compress(S_(s), (int)n_out, dst, P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out96, s->d_aux.p, 96 * n_out, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

// the field-edge hooks (k_check_canon, k_check_from_bytes, k_check_fp2_roots, batch_inv, launch_hash)
int lsg_check_canon(lsg_ctx* c, const uint32_t* in, size_t n, const uint8_t* bytes48, size_t nb, uint32_t* out,
                    uint32_t* out_limbs) {
  constexpr size_t WOUT = lsgk::CHECK_CANON_OUT;
  if (!c || (n && (!in || !out)) || (nb && (!bytes48 || !out_limbs)) || n > 0x7fffffffull / (4 * WOUT) ||
      nb > 0x7fffffffull / (4 * W_FP))
    return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  if (n) {
    LSG_RC(ensure(s, s->d_aux, 4 * W_FP * n));
    LSG_RC(ensure(s, s->d_Fb, 4 * WOUT * n));
    LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
    KL(s, "k_check_canon", lsgk::check_canon(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
    LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * WOUT * n, hipMemcpyDeviceToHost, s->st[0]));
    LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  }
  if (nb) {
    LSG_RC(ensure(s, s->d_aux, 48 * nb));
    LSG_RC(ensure(s, s->d_Fb, 4 * W_FP * nb));
    LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, bytes48, 48 * nb, hipMemcpyHostToDevice, s->st[0]));
    KL(s, "k_check_from_bytes", lsgk::check_from_bytes(S_(s), (int)nb, P_<uint8_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
    LSG_HIP(s, hipMemcpyAsync(out_limbs, s->d_Fb.p, 4 * W_FP * nb, hipMemcpyDeviceToHost, s->st[0]));
    LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  }
  return LSG_OK;
}

int lsg_check_fp2_roots(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) {
  constexpr size_t WOUT = lsgk::CHECK_ROOTS_OUT;
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * WOUT)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * 2 * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * WOUT * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * 2 * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  KL(s, "k_check_fp2_roots", lsgk::check_fp2_roots(S_(s), (int)n, P_<uint32_t>(s->d_aux), P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * WOUT * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  return LSG_OK;
}

int lsg_check_batch_inv(lsg_ctx* c, const uint32_t* in, size_t n, uint32_t* out) {
  if (!c || (n && (!in || !out)) || n > 0x7fffffffull / (4 * W_FP)) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(ensure(s, s->d_aux, 4 * W_FP * n));
  LSG_RC(ensure(s, s->d_Fb, 4 * W_FP * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_aux.p, in, 4 * W_FP * n, hipMemcpyHostToDevice, s->st[0]));
  LSG_RC(batch_inv(s, 0, "binv_check", P_<uint32_t>(s->d_aux), n, P_<uint32_t>(s->d_Fb)));
  LSG_HIP(s, hipMemcpyAsync(out, s->d_Fb.p, 4 * W_FP * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

// lsg_hash_to_g2 from the expanded messages on: the caller's 256 "uniform bytes" per item
int lsg_check_map_uniform(lsg_ctx* c, const uint8_t* ub256, size_t n, uint8_t* out192) {
  if (!c || (n && (!ub256 || !out192)) || n > 0x7fffffffull / 256) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  if (n == 0) return LSG_OK;
  Slot* s = &c->dev[0]->util;
  timer_reset(s);
  LSG_RC(size_state(s, n, 0, 1, 0));
  LSG_RC(ensure(s, s->d_aux, 192 * n));
  LSG_HIP(s, hipMemcpyAsync(s->d_ub.p, ub256, 256 * n, hipMemcpyHostToDevice, s->st[0]));
  const int nn = (int)n;
  LSG_RC(launch_hash(s, nn, P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf)));
  KL(s, "k_g2a_to_bytes",
     lsgk::g2a_to_bytes(S_(s), nn, P_<uint32_t>(s->d_H), P_<uint8_t>(s->d_hinf), P_<uint8_t>(s->d_aux)));
  LSG_HIP(s, hipMemcpyAsync(out192, s->d_aux.p, 192 * n, hipMemcpyDeviceToHost, s->st[0]));
  LSG_HIP(s, hipStreamSynchronize(s->st[0]));
  keep_times(s);
  return LSG_OK;
}

int lsg_probe_fp_mul_rate(lsg_ctx* c, double* fp_mul_per_s, double* mad_per_s) {
  if (!c || !fp_mul_per_s || !mad_per_s) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = &c->dev[0]->util;
  hipDeviceProp_t prop;
  LSG_HIP(s, hipGetDeviceProperties(&prop, c->dev[0]->device));
  const int items = prop.multiProcessorCount * 32 * 32;  // 32 waves per CU, 32 pair items each
  LSG_RC(ensure(s, s->d_aux, 4 * W_FP * (size_t)items));
  std::vector<uint32_t> init(W_FP * (size_t)items, 0);
  for (size_t i = 0; i < init.size(); i += 4) init[i] = (uint32_t)(i * 2654435761u) & 0x1fffffffu;  // small values < p
  LSG_HIP(s, hipMemcpy(s->d_aux.p, init.data(), 4 * init.size(), hipMemcpyHostToDevice));
  const int iters = 64;
  hipStream_t S = s->st[0];
  LSG_HIP(s, lsgk::probe_fp_mul(S, items, 2, P_<uint32_t>(s->d_aux)));
  hipEvent_t a, b;
  LSG_HIP(s, hipEventCreate(&a));
  LSG_HIP(s, hipEventCreate(&b));
  LSG_HIP(s, hipEventRecord(a, S));
  LSG_HIP(s, lsgk::probe_fp_mul(S, items, iters, P_<uint32_t>(s->d_aux)));
  LSG_HIP(s, hipEventRecord(b, S));
  LSG_HIP(s, hipEventSynchronize(b));
  float ms = 0;
  LSG_HIP(s, hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *fp_mul_per_s = (double)items * iters * 4.0 / (ms * 1e-3);
  *mad_per_s = *fp_mul_per_s * 300.0;
  return LSG_OK;
}

int lsg_probe_mad_peak(lsg_ctx* c, double* mad_per_s) {
  if (!c || !mad_per_s) return LSG_ERR_INVALID_ARG;
  LSG_ENTER(c);
  Slot* s = &c->dev[0]->util;
  hipDeviceProp_t prop;
  LSG_HIP(s, hipGetDeviceProperties(&prop, c->dev[0]->device));
  const int blocks = prop.multiProcessorCount * 32;  // 32 waves per CU (8 per SIMD)
  const size_t threads = (size_t)blocks * 256;
  LSG_RC(ensure(s, s->d_aux, 8 * threads));
  hipStream_t S = s->st[0];
  const int iters = 4096;
  LSG_HIP(s, lsgk::probe_mad(S, blocks, 16, 3u, P_<uint64_t>(s->d_aux)));
  hipEvent_t a, b;
  LSG_HIP(s, hipEventCreate(&a));
  LSG_HIP(s, hipEventCreate(&b));
  LSG_HIP(s, hipEventRecord(a, S));
  LSG_HIP(s, lsgk::probe_mad(S, blocks, iters, 5u, P_<uint64_t>(s->d_aux)));
  LSG_HIP(s, hipEventRecord(b, S));
  LSG_HIP(s, hipEventSynchronize(b));
  float ms = 0;
  LSG_HIP(s, hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *mad_per_s = (double)threads * iters * 16.0 / (ms * 1e-3);
  return LSG_OK;
}

int lsg_last_kernel_times(lsg_ctx* c, const char** names, double* ms, int max) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  const auto& v = c->dev[0]->last_times;
  int n = 0;
  for (size_t i = 0; i < v.size() && n < max; i++, n++) {
    if (names) names[n] = v[i].first;
    if (ms) ms[n] = v[i].second;
  }
  return n;
}

int lsg_assign_jobs(const uint32_t* job_sets, size_t n_jobs, int32_t n_devices, int32_t* owner) {
  if ((n_jobs && (!job_sets || !owner)) || n_devices < 1) return LSG_ERR_INVALID_ARG;
  assign_jobs(job_sets, n_jobs, n_devices, owner);
  return LSG_OK;
}

}  // extern "C"
