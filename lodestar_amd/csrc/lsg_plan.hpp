// lsg_plan.hpp -- the host-only policy of the verifier: how a package's jobs become RLC
// groups, how Miller items and segmented reductions are planned, and how per-job verdicts and
// the batch counters follow from group verdicts (the reference's worker.ts:30-106 rules plus
// the phases B0 / B / C1 / C2).  Small integers in, small integers out: no device, no
// environment, no Slot.  Also the two lists a package adds to the plan arena beside its groups:
// the KeyValidate list of LSG_JOB_VALIDATE_KEYS jobs (plan_validate_keys) and the per-message set
// lists of the package group (plan_msg_lists).  lsg_host.hip includes it and supplies the device
// side (launches, the `check` callable of resolve_package); how sets are staged is
// lsg_stage.hpp's, built on the types here.  tests/native/plancheck.cpp drives it on the CPU
// (tests/native/stagecheck.cpp the two lists).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string.h>

#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/lodestar_bls.h"
#include "lsg_bits.h"
#include "lsg_ssz.hpp"

namespace lsgp {

typedef std::pair<size_t, size_t> Range;        // [first, second)
typedef std::pair<int32_t, int32_t> ItemRange;  // Miller items [first, second); (-1, -1): none

// chunkifyMaximizeChunkSize (multithread/utils.ts:4-19)
inline std::vector<Range> chunkify(size_t len, size_t min_per_chunk) {
  std::vector<Range> out;
  size_t chunk_count = len / min_per_chunk;
  if (chunk_count <= 1) {
    out.push_back({0, len});
    return out;
  }
  size_t per = (len + chunk_count - 1) / chunk_count;
  for (size_t i = 0; i < len; i += per) out.push_back({i, std::min(len, i + per)});
  return out;
}

// Whole jobs per device by cumulative set count (never splits a job): job j goes
// to floor(sets_before_j * n_dev / total).
inline void assign_jobs(const uint32_t* sizes, size_t n_jobs, int n_dev, int32_t* owner) {
  uint64_t total = 0;
  for (size_t j = 0; j < n_jobs; j++) total += sizes[j];
  uint64_t before = 0;
  for (size_t j = 0; j < n_jobs; j++) {
    owner[j] = (total == 0 || n_dev <= 1) ? 0 : (int32_t)std::min<uint64_t>((uint64_t)n_dev - 1, before * (uint64_t)n_dev / total);
    before += sizes[j];
  }
}

// Window width c of a group's bucket MSM (plan_phase): per set 64/c digits (bucket
// additions), per group the 64 bit sums over 2^(c-1) buckets each.  n sets cost about
// n (64/c) + 2^(c-1) 64 G2 additions: c = 2 below 48 sets, 4 below 256, 8 from there.
inline int msm_window_bits(size_t n) { return n >= 256 ? 8 : (n >= 48 ? 4 : 2); }

// ---- segmented-reduction plans (lsgk::seg_reduce): int32 words appended to a slot's plan
// arena, uploaded once per phase
struct SegPass {
  int ips_log2 = 0, n_chunks = 0;
  size_t chunk_off = 0;  // words into the arena
  int src = 0;           // 0: the reduction's input, 1/2: tmp buffer A/B
  int tmp_out = 1;       // tmp buffer (1/2) that negative outputs go to
};
struct SegPlan {
  int op = 0;
  bool has_idx = false;
  size_t idx_off = 0;
  std::vector<SegPass> passes;
  size_t tmp_items = 0;  // per tmp buffer
};
constexpr int SEG_FOLD = 16;  // at most this many serial folds per lane pair within one pass
// Fp12 products (op 2) cost ~50 us each on one lane pair: their passes fold at most 4 terms
// per pair before the butterfly (an 8193-term package product: 17 serial products in two
// passes instead of 28)
constexpr int SEG_FOLD_FP12 = 4;
// work-bound passes (>= SEG_WIDE_PAIRS lane pairs at a wave's 32 pairs per segment): up to 64
// folds per pair
constexpr int SEG_FOLD_WIDE = 64;
constexpr size_t SEG_WIDE_PAIRS = 131072;

// The A/B switches the plans and the verdict rules depend on (lsg_ab.h).  The defaults are the
// shipped library's compile-time values; lsg_host.hip fills one per package (the A/B library
// from the environment).
struct Switches {
  bool package_group = true;   // LSG_PACKAGE_GROUP=0: phase A as one group per 16-job chunk
  bool sub_groups = true;      // LSG_SUB_GROUPS=0: a coalesced launch as one group per chunk
  bool nb_merge = true;        // LSG_NB_MERGE=0: one group per non-batchable job
  bool msg_agg = true;         // LSG_MSG_AGG=0: one Miller pair per set, not per distinct message
  size_t msm_min_group = 256;  // LSG_MSM_MIN_GROUP: smallest RLC group summed by the bucket MSM
  size_t b0_min = 64;          // LSG_B0_MIN: chunks to check from which phase B0 runs (0: off)
  size_t b0_run = 4;           // LSG_B0_RUN: consecutive chunks per phase-B0 group
  int seg_fold_wide = SEG_FOLD_WIDE;  // LSG_SEG_FOLD_WIDE
  size_t slp_items = 2048;     // LSG_SLP_ITEMS as in force (0: the serial programs are off)
  // LSG_MSM_FOLD=0: the MSM's bucket pass as k_sig_proj + k_seg_reduce<1> on plan_seg's plan
  // instead of k_msm_bucket_seg on plan_buckets'; LSG_MSM_IPS >= 0 forces the latter's ips_log2
  bool msm_fold = true;
  int msm_ips = -1;
};

// lane pairs per chunk (log2): enough that the longest segment fits one chunk of SEG_FOLD
// folds per pair (one pass), and at least a quarter of the mean length (latency: folds are
// serial, the butterfly is log2(ips) steps); at most a wave's 32 pairs
inline int ips_for(double avg, int32_t max_len, int fold) {
  int l = 0;
  while (l < 5 && ((int32_t)(fold << l) < max_len || (double)(2 << l) * 4.0 <= avg)) l++;
  return l;
}

// a pass's chunk triples by descending length (stable): chunk order is free, every chunk carries
// its output, and a wave whose chunks are alike finishes its serial folds together
inline void sort_chunks_desc(int32_t* chunks, size_t n) {
  struct Tri {
    int32_t off, len, out;
  };
  std::vector<Tri> v(n);
  for (size_t c = 0; c < n; c++) v[c] = {chunks[3 * c], chunks[3 * c + 1], chunks[3 * c + 2]};
  std::stable_sort(v.begin(), v.end(), [](const Tri& a, const Tri& b) { return a.len > b.len; });
  for (size_t c = 0; c < n; c++) {
    chunks[3 * c] = v[c].off;
    chunks[3 * c + 1] = v[c].len;
    chunks[3 * c + 2] = v[c].out;
  }
}

// Segments s = 0..ns-1: elements [seg_off[s], seg_off[s] + seg_len[s]) of the idx list (at
// idx_off in the arena; has_idx) or of the input itself; result s goes to dst[dst_base + s].
// first_ips >= 0 (plan_buckets only): the first pass takes that many lane pairs per chunk (log2),
// folds up to max(SEG_FOLD, fold_wide) members per pair and lists its chunks by descending
// length; later passes, and every pass of every other caller, are planned as ever.
inline SegPlan plan_seg(std::vector<int32_t>& A, int op, const std::vector<int32_t>& seg_off,
                        const std::vector<int32_t>& seg_len, bool has_idx, size_t idx_off, int32_t dst_base,
                        int fold_wide, int first_ips = -1) {
  SegPlan P;
  P.op = op;
  P.has_idx = has_idx;
  P.idx_off = idx_off;
  const size_t ns = seg_len.size();
  if (ns == 0) return P;
  size_t total = 0;
  for (int32_t l : seg_len) total += (size_t)l;
  // pending: (segment, element offset, length, source) still to reduce
  struct Pend {
    int32_t seg, off, len;
  };
  std::vector<Pend> cur(ns);
  for (size_t s = 0; s < ns; s++) cur[s] = {(int32_t)s, seg_off[s], seg_len[s]};
  double avg = (double)total / (double)ns;
  int src = 0, tmp_out = 1;
  while (!cur.empty()) {
    SegPass pass;
    int32_t max_len = 0;
    for (const Pend& p : cur) max_len = std::max(max_len, p.len);
    int fold = op == 2 ? SEG_FOLD_FP12 : SEG_FOLD;
    pass.ips_log2 = ips_for(avg, max_len, fold);
    // many segments (a block body's ~8k aggregations of ~450 keys): the launch is work-bound,
    // and every butterfly level costs each lane pair one operation, so use as few pairs per
    // chunk as keep the chip full, folding up to SEG_FOLD_WIDE terms each
    if (op != 2 && (cur.size() << 5) >= SEG_WIDE_PAIRS) {
      int l = 0;
      while (l < pass.ips_log2 && (int32_t)(fold_wide << l) < max_len) l++;
      pass.ips_log2 = l;
      fold = fold_wide;
    }
    const bool first_given = first_ips >= 0 && P.passes.empty();
    if (first_given) {
      pass.ips_log2 = std::min(first_ips, 5);
      fold = std::max(SEG_FOLD, fold_wide);
    }
    pass.src = src;
    pass.tmp_out = tmp_out;
    const int32_t cap = (int32_t)((1 << pass.ips_log2) * fold);
    pass.chunk_off = A.size();
    std::vector<Pend> nxt;
    int32_t t = 0;
    size_t nxt_total = 0;
    for (const Pend& p : cur) {
      if (p.len <= cap) {
        A.push_back(p.off);
        A.push_back(p.len);
        A.push_back(dst_base + p.seg);
        pass.n_chunks++;
      } else {
        const int32_t first = t;
        for (int32_t o = 0; o < p.len; o += cap) {
          A.push_back(p.off + o);
          A.push_back(std::min(cap, p.len - o));
          A.push_back(-(t + 1));
          t++;
          pass.n_chunks++;
        }
        nxt.push_back({p.seg, first, t - first});
        nxt_total += (size_t)(t - first);
      }
    }
    if (first_given) sort_chunks_desc(A.data() + pass.chunk_off, (size_t)pass.n_chunks);
    P.tmp_items = std::max(P.tmp_items, (size_t)t);
    P.passes.push_back(pass);
    avg = nxt.empty() ? 1.0 : (double)nxt_total / (double)nxt.size();
    cur.swap(nxt);
    src = tmp_out;  // the next pass reads this pass's partial results, contiguously
    tmp_out = tmp_out == 1 ? 2 : 1;
  }
  return P;
}

// ---- the bucket pass of the signature MSM (k_msm_bucket_seg): work-bound by construction.
// A pass costs every lane pair of a wave the wave's longest serial fold plus one complete
// addition per butterfly level, whether the pair's result is kept or not, so the model counts a
// pass in lane-pair additions: chunks laid out 32 >> ips_log2 per wave in launch order, a wave
// costing 32 x (its longest fold + ips_log2), a fold of m members m - 1 additions.
// bucket_cost: that count from the bucket lengths alone (sorted by descending length), for the
// plan plan_seg(..., first_ips) would make -- its choice of pairs and fold per pass restated --
// without making it; first_ips < 0: plan_seg's own plan (chunks in bucket order: `lens` as given).
struct SegCost {
  size_t adds = 0, waves = 0;  // waves: of the first pass
  int chain = 0;               // the longest dependent run of additions, summed over the passes
  int passes = 0;
};
inline SegCost bucket_cost(const std::vector<int32_t>& lens, int first_ips, int fold_wide) {
  SegCost c;
  std::vector<int32_t> split, nxt;
  const std::vector<int32_t>* cur = &lens;
  size_t total = 0;
  for (int32_t l : lens) total += (size_t)l;
  double avg = lens.empty() ? 1.0 : (double)total / (double)lens.size();
  while (!cur->empty()) {
    int32_t max_len = 0;
    for (int32_t l : *cur) max_len = std::max(max_len, l);
    int fold = SEG_FOLD, l2 = ips_for(avg, max_len, fold);
    if ((cur->size() << 5) >= SEG_WIDE_PAIRS) {
      int l = 0;
      while (l < l2 && (int32_t)(fold_wide << l) < max_len) l++;
      l2 = l;
      fold = fold_wide;
    }
    const bool given = first_ips >= 0 && c.passes == 0;
    if (given) {
      l2 = std::min(first_ips, 5);
      fold = std::max(SEG_FOLD, fold_wide);
    }
    const int32_t cap = (int32_t)(fold << l2), ips = 1 << l2;
    const std::vector<int32_t>* chunks = cur;
    std::vector<int32_t> pieces;
    if (max_len > cap) {  // (rare: a bucket longer than a chunk)
      split.clear();
      size_t nt = 0;
      for (int32_t l : *cur) {
        if (l <= cap) {
          split.push_back(l);
          continue;
        }
        for (int32_t o = 0; o < l; o += cap) split.push_back(std::min(cap, l - o));
        pieces.push_back((l + cap - 1) / cap);
        nt += (size_t)pieces.back();
      }
      if (given) std::sort(split.begin(), split.end(), std::greater<int32_t>());
      chunks = &split;
      avg = pieces.empty() ? 1.0 : (double)nt / (double)pieces.size();
    }
    const size_t per_wave = (size_t)32 >> l2, n = chunks->size();
    int pass_chain = 0;
    size_t waves = 0;
    for (size_t w = 0; w < n; w += per_wave, waves++) {
      int32_t longest = (*chunks)[w];
      if (!given || chunks != &lens)  // (not known to be sorted: look at the whole wave)
        for (size_t k = w; k < std::min(n, w + per_wave); k++) longest = std::max(longest, (*chunks)[k]);
      const int cost = (longest > 0 ? (int)((longest + ips - 1) / ips) - 1 : 0) + l2;
      c.adds += (size_t)32 * (size_t)cost;
      pass_chain = std::max(pass_chain, cost);
    }
    if (c.passes == 0) c.waves = waves;
    c.chain += pass_chain;
    c.passes++;
    nxt.swap(pieces);
    cur = &nxt;
    if (nxt.empty()) break;
  }
  return c;
}
// The first pass takes the candidate ips_log2 in 0..5 with the most lane pairs whose modelled cost
// is within BUCKET_COST_TOL of the cheapest candidate's: more pairs per bucket shorten the chain
// of dependent additions, and the tolerance is what that may cost in instructions.  A candidate
// that takes more passes than plan_seg's own plan -- a pass is a launch and a round trip through
// memory -- is none; 32 pairs per bucket never does.  A pass that is both narrow and long -- fewer
// than BUCKET_MIN_WAVES waves, more than the SEG_FOLD dependent additions plan_seg allows any
// pass -- is latency-bound however little it costs, so it widens while the passes stay the same.
// The constants come from the sweep in DESIGN.md section 5l.  The tolerance is bracketed there by
// two workloads; the floor rests on one (committees at 255 waves, inside a wide spread), and it
// does not act on chains of SEG_FOLD or fewer, so it is weakly supported.
// Where no bucket holds more than SEG_FOLD members (a group of a few hundred sets: about one
// member per bucket) there is no butterfly to save and nothing to price: the pass keeps
// plan_seg's plan as it is, and such a group costs the host nothing new.
constexpr double BUCKET_COST_TOL = 1.25;
constexpr size_t BUCKET_MIN_WAVES = 256;
// force_ips >= 0 (the A/B library's LSG_MSM_IPS): that candidate, whatever the model says
inline int bucket_ips(const std::vector<int32_t>& seg_len, int fold_wide) {
  const int max_passes = bucket_cost(seg_len, -1, fold_wide).passes;
  std::vector<int32_t> lens(seg_len);
  std::sort(lens.begin(), lens.end(), std::greater<int32_t>());
  SegCost cost[6];
  size_t best = ~(size_t)0;
  for (int l = 0; l <= 5; l++) {
    cost[l] = bucket_cost(lens, l, fold_wide);
    if (cost[l].passes <= max_passes) best = std::min(best, cost[l].adds);
  }
  int pick = 5;
  for (int l = 0; l <= 5; l++)
    if (cost[l].passes <= max_passes && (double)cost[l].adds <= BUCKET_COST_TOL * (double)best) pick = l;
  while (pick < 5 && cost[pick].waves < BUCKET_MIN_WAVES && cost[pick].chain > SEG_FOLD &&
         cost[pick + 1].passes == cost[pick].passes)
    pick++;
  return pick;
}
inline SegPlan plan_buckets(std::vector<int32_t>& A, const std::vector<int32_t>& seg_off,
                            const std::vector<int32_t>& seg_len, size_t idx_off, int fold_wide, int force_ips = -1) {
  if (force_ips < 0) {
    int32_t max_len = 0;
    for (int32_t l : seg_len) max_len = std::max(max_len, l);
    if (max_len <= SEG_FOLD) return plan_seg(A, 1, seg_off, seg_len, true, idx_off, 0, fold_wide);
  }
  const int pick = force_ips >= 0 ? std::min(force_ips, 5) : bucket_ips(seg_len, fold_wide);
  return plan_seg(A, 1, seg_off, seg_len, true, idx_off, 0, fold_wide, pick);
}

// One RLC group: sets [first, first + len) (a contiguous range: the package group, one
// non-batchable job, one 16-job chunk or one job).
struct Grp {
  size_t first = 0, len = 0;
  bool msm = false;
};

// Sets of group g that share a message share one Miller pair (msg_agg): per distinct message
// (msg_id[i]: set i's, n_msgs of them) the list of g's sets that sign it, appended to the arena
// in set order, and the segmented sum (op 0) over those lists, result j = message j's.
inline SegPlan plan_msg_lists(std::vector<int32_t>& A, const uint32_t* msg_id, size_t n_msgs, const Grp& g,
                              int fold_wide) {
  std::vector<int32_t> cnt(n_msgs, 0), off(n_msgs), fill;
  for (size_t i = g.first; i < g.first + g.len; i++) cnt[msg_id[i]]++;
  int32_t tot = 0;
  for (size_t j = 0; j < n_msgs; j++) {
    off[j] = tot;
    tot += cnt[j];
  }
  fill = off;
  const size_t idx_off = A.size();
  A.resize(idx_off + (size_t)tot);
  for (size_t i = g.first; i < g.first + g.len; i++) A[idx_off + (size_t)fill[msg_id[i]]++] = (int32_t)i;
  return plan_seg(A, 0, off, cnt, true, idx_off, 0, fold_wide);
}

// ---- group stages of one phase (no host synchronisation).  Groups with msm sum their
// signatures by the bucket MSM over the unscaled points in d_rs (MSM groups must come first);
// the rest sum the scaled points in rs.  Then per group ML(-G1, S_g) on a row, the product
// with the group's Miller items (fall: items [0, n_items) followed by one slot per group),
// the canonical product F_g (d_Fb, D2H into h_blob when export), and FE(F_g) into d_verdict.
struct PhasePlan {
  std::vector<Grp> groups;
  size_t n_msm = 0;
  SegPlan buckets, bits, sums, prod;
  size_t n_items = 0;   // Miller items of the phase's groups (fall slots 0 .. n_items-1)
  size_t item_off = 0;  // item_first / item_cnt in the plan arena
  size_t term_base = 0;  // fall slot of group g's ML(-G1, S_g) term: term_base + g
  // per group, optional set sub-ranges items must not cross (the package group's 16-job
  // chunks); sub_items = the item range of every sub-range, in order
  std::vector<std::vector<Range>> sub;
  std::vector<ItemRange> sub_items;
  // reuse: the groups' products take their items from an earlier phase (given item ranges)
  bool reuse_items = false;
  std::vector<ItemRange> given;
  // host copy of the items (first set, set count): phase C's item-aligned job groups
  std::vector<int32_t> it_first, it_cnt;
  bool single_items = false;  // every item is one set: the list form of the Miller loop runs
  // one Miller pair per distinct message for group agg_g (>= 0): its items are the n_magg
  // message items (plan arena at magg_off) after the n_set_items per-set items
  int agg_g = -1;
  size_t n_magg = 0, magg_off = 0, n_set_items = 0;
};

// ---- Miller items: <= K consecutive sets of one range (group); item_first / item_cnt go to
// the arena A.  Returns the number of items; range_items (optional): per range, its items.
inline size_t plan_items(std::vector<int32_t>& A, size_t K, const std::vector<Range>& ranges, size_t* off,
                         std::vector<ItemRange>* range_items, std::vector<int32_t>* host_first,
                         std::vector<int32_t>* host_cnt) {
  std::vector<int32_t> first, cnt;
  for (auto& r : ranges) {
    const int32_t i0 = (int32_t)first.size();
    for (size_t i = r.first; i < r.second; i += K) {
      first.push_back((int32_t)i);
      cnt.push_back((int32_t)std::min(K, r.second - i));
    }
    if (range_items) range_items->push_back({i0, (int32_t)first.size()});
  }
  *off = A.size();
  A.insert(A.end(), first.begin(), first.end());
  A.insert(A.end(), cnt.begin(), cnt.end());
  if (host_first) *host_first = first;
  if (host_cnt) *host_cnt = cnt;
  return first.size();
}

// The reductions of one phase into the arena A: bucket MSM (rnd: the per-set randomizers) or
// scaled sums per group, the phase's Miller items (K pairs each) and the groups' products.
inline void plan_phase(std::vector<int32_t>& A, const std::vector<uint64_t>& rnd, int K, const Switches& sw,
                       PhasePlan& Ph) {
  const size_t ng = Ph.groups.size();
  Ph.n_msm = 0;
  while (Ph.n_msm < ng && Ph.groups[Ph.n_msm].msm) Ph.n_msm++;
  // bucket MSM: per MSM group, bucket (w, d) = the sets whose w-th c-bit digit of r_i is d.
  // c = 8 (8 windows x 255 buckets) for large groups; c = 4 (16 x 15) below MSM_C8_MIN sets,
  // where 2040 buckets' bit sums would cost more than the sets' bucket additions (a block's
  // 128-set groups: 16 additions per set + 512 per group instead of a 64-bit scalar
  // multiplication per set).  Buckets are numbered compactly (group bases); bit k = c w + j
  // sums the buckets (w, d) whose digit d has bit j set, so every group has 64 bit sums and
  // one Horner program whatever its c.
  if (Ph.n_msm) {
    std::vector<int> cw(Ph.n_msm);
    std::vector<size_t> gbase(Ph.n_msm + 1, 0);
    for (size_t g = 0; g < Ph.n_msm; g++) {
      cw[g] = msm_window_bits(Ph.groups[g].len);
      gbase[g + 1] = gbase[g] + (size_t)(64 / cw[g]) * (size_t)((1u << cw[g]) - 1);
    }
    auto bucket = [&](size_t g, int w, uint32_t d) { return gbase[g] + (size_t)w * ((1u << cw[g]) - 1) + d - 1; };
    std::vector<int32_t> cnt(gbase[Ph.n_msm], 0);
    for (size_t g = 0; g < Ph.n_msm; g++) {
      const int c = cw[g], nw = 64 / c;
      const uint64_t dm = (1ull << c) - 1;
      for (size_t i = Ph.groups[g].first; i < Ph.groups[g].first + Ph.groups[g].len; i++) {
        const uint64_t r = rnd[i];
        for (int w = 0; w < nw; w++) {
          const uint32_t d = (uint32_t)((r >> (c * w)) & dm);
          if (d) cnt[bucket(g, w, d)]++;
        }
      }
    }
    std::vector<int32_t> seg_off(cnt.size()), seg_len(cnt);
    int32_t tot = 0;
    for (size_t b = 0; b < cnt.size(); b++) {
      seg_off[b] = tot;
      tot += cnt[b];
    }
    const size_t idx_off = A.size();
    A.resize(idx_off + (size_t)tot);
    int32_t* idx = A.data() + idx_off;
    std::vector<int32_t> fill(seg_off);
    for (size_t g = 0; g < Ph.n_msm; g++) {
      const int c = cw[g], nw = 64 / c;
      const uint64_t dm = (1ull << c) - 1;
      for (size_t i = Ph.groups[g].first; i < Ph.groups[g].first + Ph.groups[g].len; i++) {
        const uint64_t r = rnd[i];
        for (int w = 0; w < nw; w++) {
          const uint32_t d = (uint32_t)((r >> (c * w)) & dm);
          if (d) idx[fill[bucket(g, w, d)]++] = (int32_t)i;
        }
      }
    }
    Ph.buckets = sw.msm_fold ? plan_buckets(A, seg_off, seg_len, idx_off, sw.seg_fold_wide, sw.msm_ips)
                             : plan_seg(A, 1, seg_off, seg_len, true, idx_off, 0, sw.seg_fold_wide);
    // bit (g, k = c w + j): the buckets (g, w, d) whose digit d has bit j set
    const size_t bidx = A.size();
    std::vector<int32_t> boff, blen;
    for (size_t g = 0; g < Ph.n_msm; g++) {
      const int c = cw[g], nw = 64 / c;
      for (int w = 0; w < nw; w++)
        for (int j = 0; j < c; j++) {
          boff.push_back((int32_t)(A.size() - bidx));
          for (uint32_t d = 1; d < (1u << c); d++)
            if ((d >> j) & 1u) A.push_back((int32_t)bucket(g, w, d));
          blen.push_back((int32_t)(A.size() - bidx) - boff.back());
        }
    }
    Ph.bits = plan_seg(A, 1, boff, blen, true, bidx, 0, sw.seg_fold_wide);
  }
  // scaled groups: S_g = sum of the contiguous scaled points
  if (Ph.n_msm < ng) {
    std::vector<int32_t> off, len;
    for (size_t g = Ph.n_msm; g < ng; g++) {
      off.push_back((int32_t)Ph.groups[g].first);
      len.push_back((int32_t)Ph.groups[g].len);
    }
    Ph.sums = plan_seg(A, 1, off, len, false, 0, (int32_t)Ph.n_msm, sw.seg_fold_wide);
  }
  // Miller items of this phase: <= K consecutive sets, never crossing a group (nor one of its
  // sub-ranges), unless the groups reuse an earlier phase's items
  std::vector<ItemRange> gi;
  if (Ph.reuse_items) {
    gi = Ph.given;
  } else {
    std::vector<Range> ranges;
    std::vector<size_t> nsub(ng, 1);
    for (size_t g = 0; g < ng; g++) {
      if ((int)g == Ph.agg_g) {  // message items instead (below)
        nsub[g] = 0;
      } else if (g < Ph.sub.size() && !Ph.sub[g].empty()) {
        ranges.insert(ranges.end(), Ph.sub[g].begin(), Ph.sub[g].end());
        nsub[g] = Ph.sub[g].size();
      } else {
        ranges.push_back({Ph.groups[g].first, Ph.groups[g].first + Ph.groups[g].len});
      }
    }
    Ph.sub_items.clear();
    Ph.n_items = plan_items(A, (size_t)K, ranges, &Ph.item_off, &Ph.sub_items, &Ph.it_first, &Ph.it_cnt);
    Ph.single_items = true;
    for (int32_t c : Ph.it_cnt) Ph.single_items = Ph.single_items && c == 1;
    Ph.n_set_items = Ph.n_items;
    if (Ph.agg_g >= 0) {  // item n_set_items + j = message j (one pair)
      Ph.magg_off = A.size();
      for (size_t j = 0; j < Ph.n_magg; j++) A.push_back((int32_t)j);
      for (size_t j = 0; j < Ph.n_magg; j++) A.push_back(1);
      Ph.n_items += Ph.n_magg;
    }
    Ph.term_base = Ph.n_items;
    size_t r = 0;
    for (size_t g = 0; g < ng; g++) {
      if ((int)g == Ph.agg_g) {
        gi.push_back({(int32_t)Ph.n_set_items, (int32_t)Ph.n_items});
        continue;
      }
      gi.push_back({Ph.sub_items[r].first, Ph.sub_items[r + nsub[g] - 1].second});
      r += nsub[g];
    }
  }
  // F_g = f_g * prod of the group's items; element ids index fall
  const size_t pidx = A.size();
  std::vector<int32_t> poff, plen;
  for (size_t g = 0; g < ng; g++) {
    poff.push_back((int32_t)(A.size() - pidx));
    for (int32_t it = gi[g].first; it < gi[g].second; it++) A.push_back(it);
    A.push_back((int32_t)(Ph.term_base + g));
    plen.push_back((int32_t)(A.size() - pidx) - poff.back());
  }
  Ph.prod = plan_seg(A, 2, poff, plen, true, pidx, 0, sw.seg_fold_wide);
}

// ---- messages given as an SSZ object + domain (LSG_MSG_OBJECT)
// A marked length word is marker (bit 31), kind tag (bits 24..30), payload length (bits 0..23);
// an unmarked one is a byte count in all its bits.
inline bool msg_marked(uint32_t msg_len) { return (msg_len & LSG_MSG_OBJECT) != 0; }
// the bytes behind lsg_set.msg
inline uint32_t msg_bytes(uint32_t msg_len) {
  return msg_marked(msg_len) ? msg_len & ~(LSG_MSG_OBJECT | LSG_MSG_KIND_MASK) : msg_len;
}
// the kind tag of a marked length (0: the kind is selected by the payload length, or unmarked)
inline uint32_t msg_kind_tag(uint32_t msg_len) {
  return msg_marked(msg_len) ? (msg_len & LSG_MSG_KIND_MASK) >> LSG_MSG_KIND_SHIFT : 0;
}
// marked with tag 0: one of the fixed-size kinds, k_msg_roots' work
inline bool msg_fixed_object(uint32_t msg_len) { return msg_marked(msg_len) && !msg_kind_tag(msg_len); }
// The object's serialized length (the kind, as ssz_object_signing_root of lsg_ssz.hpp takes it)
// that a marked msg_len with tag 0 selects by its payload length, object + 32-byte domain; 0:
// none -- an unmarked length, a tagged one, or a payload length outside the table.
inline uint32_t msg_object_kind(uint32_t msg_len) {
  if (!msg_marked(msg_len) || msg_kind_tag(msg_len)) return 0;
  switch (msg_bytes(msg_len)) {
    case 40: return 8;     // uint64
    case 48: return 16;    // two uint64 fields
    case 64: return 32;    // Root
    case 108: return 76;   // capella.BLSToExecutionChange
    case 120: return 88;   // phase0.DepositMessage
    case 144: return 112;  // phase0.BeaconBlockHeader
    case 160: return 128;  // phase0.AttestationData
    case 296: return 264;  // altair.ContributionAndProof
    default: return 0;
  }
}
// The structure of a variable-size object (kind tag 1: phase0.AggregateAndProof, 2: EIP-7549's;
// the layout is lsg_ssz.hpp's, whose device text assumes what is checked here): the length in
// range, both offsets as the fixed parts dictate, a delimiter bit in the last byte, and no more
// bits than the list's limit.  obj: obj_len readable bytes.
inline bool msg_var_ok(uint32_t kind, const uint8_t* obj, size_t obj_len) {
  if ((kind != LSG_MSG_KIND_AGG_PROOF && kind != LSG_MSG_KIND_AGG_PROOF_ELECTRA) || !obj) return false;
  const uint32_t off = ssz_var_bits_off(kind), max_bits = ssz_var_max_bits(kind);
  if (obj_len <= off || obj_len > off + max_bits / 8 + 1) return false;
  uint32_t o1, o2;
  memcpy(&o1, obj + 8, 4);  // (little-endian hosts, as the rest of the staging)
  memcpy(&o2, obj + 108, 4);
  if (o1 != 108 || o2 != off - 108) return false;
  const uint8_t last = obj[obj_len - 1];
  return last != 0 && ssz_var_shape(kind, (uint32_t)obj_len, last).n_bits <= max_bits;
}
// A marked set must select a kind and carry its bytes, a tagged one well-formed: anything else
// is a caller bug, answered with LSG_ERR_INVALID_ARG before a slot is taken.  Unmarked sets
// pass as they are.
inline bool msg_set_ok(const lsg_set& t) {
  if (!msg_marked(t.msg_len)) return true;
  if (!t.msg) return false;
  const uint32_t tag = msg_kind_tag(t.msg_len), mb = msg_bytes(t.msg_len);
  if (!tag) return msg_object_kind(t.msg_len) != 0;
  return mb > 32 && msg_var_ok(tag, t.msg, mb - 32);
}
// Likewise a multi-committee set (LSG_PK_BITS_MULTI) without a blob, or listing more than
// LSG_MAX_SET_COMMITTEES committees.  multi_k: the blob's leading count.
inline uint32_t multi_k(const lsg_set& t) {
  uint32_t k = 0;
  memcpy(&k, t.pks, 4);
  return k;
}
inline bool multi_set_ok(const lsg_set& t) {
  return t.pk_len != LSG_PK_BITS_MULTI || (t.pks && multi_k(t) <= LSG_MAX_SET_COMMITTEES);
}
inline bool msg_sets_ok(const lsg_set* sets, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!msg_set_ok(sets[i]) || !multi_set_ok(sets[i])) return false;
  return true;
}
inline bool msg_jobs_ok(const lsg_job* jobs, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; j++)
    if (jobs[j].n_sets && jobs[j].sets && !msg_sets_ok(jobs[j].sets, jobs[j].n_sets)) return false;
  return true;
}

// ---- one device's share of a package
struct JobRec {
  size_t first = 0, count = 0;  // staged set range
  uint32_t flags = 0;
};

struct PkgShape {
  std::vector<JobRec> jobs;         // this device's share of the package, caller order
  std::vector<size_t> job_ids;      // caller job index of jobs[k]
  std::vector<size_t> batch_order;  // indices into jobs: batchable jobs in staging order
  size_t nb_sets = 0;               // sets of the batchable jobs (staged first)
  // coalesced launch (lsg_set_coalesce): n_sub caller packages in one slot.  sub_first: their
  // job-index bounds in the merged job list; bpos_first: their bounds in batch_order.  Each
  // one keeps its own 16-job chunks, deserialisation rule and counters.
  int n_sub = 0;
  std::vector<size_t> sub_first, bpos_first;
  // per staged set: its key count and first key; kv_set[i] != 0: set i's keys are validated on
  // the device (LSG_JOB_VALIDATE_KEYS; empty when the package has no such key)
  std::vector<uint32_t> pk_cnt, pk_first;
  std::vector<uint8_t> kv_set;
  // sets whose keys are a committee id + participation bits (LSG_PK_BITS; both empty when the
  // package has none): bits_p[i] = the set's participant count, -1 for a set of another kind
  // (such a set stages no key slots: pk_cnt[i] == 0); bits_kerr[i] = its set-level key error
  // resolved on the host (LSG_ERR_BAD_COMMITTEE), routed like a key that does not deserialize
  std::vector<int32_t> bits_p, bits_kerr;
};

// Staging order of jobs `ids` of `jobs` (batchable jobs first, each kind in caller order) and
// the sub-package bounds `subs` of a coalesced launch (null: one package).  Returns the number
// of sets; the per-set fields are the stager's.
inline size_t shape_jobs(PkgShape& sh, const lsg_job* jobs, const std::vector<size_t>& ids,
                         const std::vector<size_t>* subs) {
  const size_t nj = ids.size();
  sh.jobs.assign(nj, JobRec());
  sh.job_ids = ids;
  sh.batch_order.clear();
  size_t n = 0;
  for (int pass = 0; pass < 2; pass++)
    for (size_t k = 0; k < nj; k++) {
      const lsg_job& J = jobs[ids[k]];
      const bool b = (J.flags & LSG_JOB_BATCHABLE) != 0;
      if (b != (pass == 0)) continue;
      sh.jobs[k].first = n;
      sh.jobs[k].count = J.n_sets;
      sh.jobs[k].flags = J.flags;
      n += J.n_sets;
      if (b) sh.batch_order.push_back(k);
    }
  sh.nb_sets = 0;
  for (size_t k : sh.batch_order) sh.nb_sets += sh.jobs[k].count;
  sh.n_sub = subs ? (int)subs->size() - 1 : 0;
  sh.sub_first.clear();
  sh.bpos_first.clear();
  if (subs) {
    sh.sub_first = *subs;
    sh.bpos_first.assign(1, 0);
    size_t q = 0;
    for (int k = 0; k < sh.n_sub; k++) {
      while (q < sh.batch_order.size() && sh.batch_order[q] < (*subs)[(size_t)k + 1]) q++;
      sh.bpos_first.push_back(q);
    }
  }
  return n;
}

inline bool batchable(const JobRec& J) { return (J.flags & LSG_JOB_BATCHABLE) != 0; }

// the 16-job chunks (worker.ts:51) of the batchable jobs as batch_order positions: over the
// whole package, or per sub-package of a coalesced launch (never across two)
inline std::vector<Range> pkg_chunks(const PkgShape& sh) {
  if (sh.n_sub == 0) return chunkify(sh.batch_order.size(), 16);
  std::vector<Range> out;
  for (int k = 0; k < sh.n_sub; k++) {
    const size_t a = sh.bpos_first[(size_t)k], b = sh.bpos_first[(size_t)k + 1];
    if (b == a) continue;
    for (auto& c : chunkify(b - a, 16)) out.push_back({a + c.first, a + c.second});
  }
  return out;
}
// sub-package of a batch_order position / of a job (coalesced launches; 0 otherwise)
inline int sub_of_pos(const PkgShape& sh, size_t q) {
  if (sh.n_sub == 0) return 0;
  return (int)(std::upper_bound(sh.bpos_first.begin(), sh.bpos_first.end(), q) - sh.bpos_first.begin()) - 1;
}
inline int sub_of_job(const PkgShape& sh, size_t j) {
  if (sh.n_sub == 0) return 0;
  return (int)(std::upper_bound(sh.sub_first.begin(), sh.sub_first.end(), j) - sh.sub_first.begin()) - 1;
}
// The sets of batch_order positions [r.first, r.second) (a chunk, a sub-package) as one group:
// batchable jobs are staged back to back in batch_order, so the range is contiguous.
inline Grp pos_sets(const PkgShape& sh, Range r) {
  Grp g;
  if (r.first < r.second) g.first = sh.jobs[sh.batch_order[r.first]].first;
  for (size_t q = r.first; q < r.second; q++) g.len += sh.jobs[sh.batch_order[q]].count;
  return g;
}
inline Grp job_sets(const JobRec& J) {
  Grp g;
  g.first = J.first;
  g.len = J.count;
  return g;
}

// ---- per-set status read back from the device
struct SetStatus {
  const int32_t* err = nullptr;    // per set: BLST code (0 ok)
  std::vector<uint8_t> pinf;       // per set: aggregated pk is infinity (2: no keys at all)
  const int32_t* pkerr = nullptr;  // per pubkey
};

inline int32_t set_error(const SetStatus& ss, size_t i) {
  if (ss.err[i]) return ss.err[i];
  if (ss.pinf[i] == 2) return LSG_ERR_EMPTY_AGGREGATE;
  return ss.pinf[i] ? LSG_BLST_PK_IS_INFINITY : 0;
}

// Error a job's maybeBatch call would throw, in the reference's order:
// Signature.fromBytes over all sets first (maybeBatch.ts:17-26 map), then
// mul_n_aggregate rejecting an infinite public key (BLST_PK_IS_INFINITY).
inline int32_t job_error(const SetStatus& ss, size_t first, size_t count) {
  if (count == 0) return LSG_ERR_EMPTY_SET;
  for (size_t k = 0; k < count; k++)
    if (ss.err[first + k]) return ss.err[first + k];
  for (size_t k = 0; k < count; k++)
    if (ss.pinf[first + k]) return set_error(ss, first + k);
  return 0;
}

// worker.ts:41-43: deserializeSet runs over the jobs in caller order before any verification;
// the first bad pubkey throws out of verifyManySignatureSets.  The code of the first bad key
// of jobs [j0, j1) (0: none) and its job in *job; a validated key (kv_set) fails its set only.
inline int32_t first_key_error(const PkgShape& sh, const int32_t* pkerr, size_t j0, size_t j1, size_t* job) {
  for (size_t k = j0; k < j1; k++) {  // jobs[k] are in caller order (job_ids ascending)
    const JobRec& J = sh.jobs[k];
    for (size_t i = J.first; i < J.first + J.count; i++) {
      if (!sh.kv_set.empty() && sh.kv_set[i]) continue;
      if (!sh.bits_kerr.empty() && sh.bits_kerr[i]) {
        *job = k;
        return sh.bits_kerr[i];
      }
      for (uint32_t q = 0; q < sh.pk_cnt[i]; q++)
        if (const int32_t e = pkerr[sh.pk_first[i] + q]) {
          *job = k;
          return e;
        }
    }
  }
  return 0;
}

// KeyValidate of the byte keys of LSG_JOB_VALIDATE_KEYS jobs (table rows were validated when
// the node cached them: the flag leaves index keys alone, and sets given by committee bits).  sets: the staged sets in staging order, sh.pk_cnt / pk_first theirs.  Sets
// sh.kv_set (empty when no key is listed) and appends the list to the arena at *kv_off: the n
// staged keys in staging order (a set's keys are adjacent), then the set of each.  Returns n.
inline size_t plan_validate_keys(PkgShape& sh, const lsg_set* const* sets, size_t n_sets, std::vector<int32_t>& A,
                                 size_t* kv_off) {
  sh.kv_set.clear();
  bool any_kv = false;
  for (size_t k = 0; k < sh.jobs.size() && !any_kv; k++) any_kv = (sh.jobs[k].flags & LSG_JOB_VALIDATE_KEYS) != 0;
  if (!any_kv) return 0;
  size_t n_kv = 0;
  sh.kv_set.assign(n_sets, 0);
  for (const JobRec& J : sh.jobs) {
    if (!(J.flags & LSG_JOB_VALIDATE_KEYS)) continue;
    for (size_t i = J.first; i < J.first + J.count; i++)
      if (sets[i]->pk_len != LSG_PK_INDEX && sets[i]->pk_len != LSG_PK_BITS && sets[i]->pk_len != LSG_PK_BITS_MULTI &&
          sh.pk_cnt[i]) {
        sh.kv_set[i] = 1;
        n_kv += sh.pk_cnt[i];
      }
  }
  *kv_off = A.size();
  A.resize(*kv_off + 2 * n_kv);
  size_t q = 0;
  for (size_t i = 0; i < n_sets; i++)
    for (uint32_t k = 0; sh.kv_set[i] && k < sh.pk_cnt[i]; k++, q++) {
      A[*kv_off + q] = (int32_t)(sh.pk_first[i] + k);
      A[*kv_off + n_kv + q] = (int32_t)i;
    }
  if (!n_kv) sh.kv_set.clear();
  return n_kv;
}

// ---- committee-resident keys: a set given as committee id + participation
// bits (LSG_PK_BITS).  The device holds every registered committee's index row and its full
// sum; a set's aggregate is either the sum of its participants (direct mode) or the committee
// sum minus the sum of its absentees (complement mode), whichever takes fewer additions.
//
// Limits of lsg_committees_set
constexpr uint32_t COMMITTEE_MAX_ID = 1u << 20;   // ids are below this
constexpr uint32_t COMMITTEE_MAX_LEN = 131072;    // members per committee

// Mode rule: p participants among n_bits, a = n_bits - p absentees.  Complement mode costs a
// mixed additions plus the final full addition with the committee sum, direct mode p.
inline bool bits_complement(uint32_t n_bits, uint32_t p) { return (uint64_t)(n_bits - p) + 1 < (uint64_t)p; }
inline uint32_t bits_wanted(uint32_t n_bits, uint32_t p) { return bits_complement(n_bits, p) ? n_bits - p : p; }

// Lane pairs of one set (log2): each pair folds at most `fold` wanted members serially before
// the butterfly, up to a wave's 32 pairs (a set never straddles a wave); beyond 32 * fold wanted
// members the serial fold grows instead.  fold is BITS_FOLD (~5 absentees: 2 pairs) unless the
// launch is work-bound, as in plan_seg: while the sets together would take more than
// BITS_WIDE_PAIRS lane pairs, every butterfly level costs each of them one full addition the
// chip has no idle lanes for, so the fold doubles, up to BITS_FOLD_WIDE (plan_bits).
constexpr int BITS_FOLD = 4;
constexpr int BITS_FOLD_WIDE = 64;
constexpr size_t BITS_WIDE_PAIRS = SEG_WIDE_PAIRS;
constexpr int BITS_MAX_PAIRS_LOG2 = 5;
inline int bits_pairs_log2(uint32_t wanted, int fold = BITS_FOLD) {
  int l = 0;
  while (l < BITS_MAX_PAIRS_LOG2 && ((uint32_t)fold << l) < wanted) l++;
  return l;
}

// Staged bit arena: set after set, each field starting on a 32-bit word and taking
// ceil(n_bits / 32) words (lsg_bits.h: the caller's bytes as they are, the tail of the last
// word zeroed).  Hosts are little-endian, as the device is.
inline size_t bits_words(uint32_t n_bits) { return ((size_t)n_bits + 31) >> 5; }
inline void bits_stage(uint32_t* dst, const uint8_t* src, uint32_t n_bits) {
  const size_t nw = bits_words(n_bits), nb = ((size_t)n_bits + 7) >> 3;
  if (nw) dst[nw - 1] = 0;
  if (nb) memcpy(dst, src, nb);
}
// participants: set bits among the first n_bits of an SSZ bitvector
inline uint32_t bits_count(const uint8_t* src, uint32_t n_bits) {
  uint32_t p = 0;
  const size_t full = n_bits >> 3;
  for (size_t k = 0; k < full; k++) p += (uint32_t)__builtin_popcount(src[k]);
  if (n_bits & 7) p += (uint32_t)__builtin_popcount(src[full] & ((1u << (n_bits & 7)) - 1u));
  return p;
}

// One bits set as staged: n_bits == 0 means "write the identity" (a set whose error the host
// already knows, or with no participant).
struct BitsSet {
  uint32_t committee = 0;
  uint32_t word_off = 0;  // its field's first word in the bit arena
  uint32_t n_bits = 0;
  uint32_t p = 0;         // participants
  int32_t out = 0;        // aggregate slot (the set's staging position)
};
// A set of a registered committee as the stager records it: its field appended to the arena
// (*words in use) -- or, with no participant, the identity entry and nothing staged.
inline BitsSet bits_stage_set(uint32_t committee, const uint8_t* bits, uint32_t n_bits, int32_t out, uint32_t* arena,
                              size_t* words) {
  BitsSet b;
  b.out = out;
  const uint32_t p = bits_count(bits, n_bits);
  if (!p) return b;
  b.committee = committee;
  b.word_off = (uint32_t)*words;
  b.n_bits = n_bits;
  b.p = p;
  bits_stage(arena + *words, bits, n_bits);
  *words += bits_words(n_bits);
  return b;
}
// Per-set plan words of k_pk_agg_bits: committee id, arena word offset, n_bits, mode (bit 0:
// complement) | pairs log2 << 8, output slot, first lane pair.
constexpr int BITS_PLAN_WORDS = LSG_BITS_PLAN_WORDS;
struct BitsPlan {
  size_t n_sets = 0, n_pairs = 0;
  int fold = BITS_FOLD;  // serial folds per lane pair the widths were chosen for
  size_t plan_off = 0;  // n_sets x BITS_PLAN_WORDS words in the arena
  size_t pair_off = 0;  // n_pairs words: the plan entry each lane pair works for
};
// Sets are laid out over the launch's lane pairs widest first, so every set starts on a
// multiple of its own (power of two) width: it never straddles a wave and its butterfly
// partners are its own pairs.
inline BitsPlan plan_bits(std::vector<int32_t>& A, const std::vector<BitsSet>& sets) {
  BitsPlan P;
  P.n_sets = sets.size();
  if (sets.empty()) return P;
  std::vector<uint32_t> order(sets.size());
  std::vector<int> lg(sets.size());
  for (;; P.fold *= 2) {
    size_t pairs = 0;
    for (size_t i = 0; i < sets.size(); i++) {
      order[i] = (uint32_t)i;
      lg[i] = sets[i].n_bits ? bits_pairs_log2(bits_wanted(sets[i].n_bits, sets[i].p), P.fold) : 0;
      pairs += (size_t)1 << lg[i];
    }
    if (pairs <= BITS_WIDE_PAIRS || P.fold >= BITS_FOLD_WIDE) break;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lg[a] > lg[b]; });
  P.plan_off = A.size();
  size_t pair = 0;
  for (uint32_t i : order) {
    const BitsSet& b = sets[i];
    A.push_back((int32_t)b.committee);
    A.push_back((int32_t)b.word_off);
    A.push_back((int32_t)b.n_bits);
    A.push_back((b.n_bits && bits_complement(b.n_bits, b.p) ? 1 : 0) | (lg[i] << 8));
    A.push_back(b.out);
    A.push_back((int32_t)pair);
    pair += (size_t)1 << lg[i];
  }
  P.n_pairs = pair;
  P.pair_off = A.size();
  for (size_t e = 0; e < order.size(); e++) A.insert(A.end(), (size_t)1 << lg[order[e]], (int32_t)e);
  return P;
}

// ---- sets spanning several committees (LSG_PK_BITS_MULTI): a committee list + one bitfield
// over the concatenation of the listed committees (an EIP-7549 aggregate).  The set is k parts,
// one per listed committee; part c's sub-field starts at bit off_c of the caller's field --
// generally not on a word boundary -- and is copied, shifted, into its own word-aligned run of
// the bit arena, so the walk of lsg_bits.h runs on a part unchanged.  Each part has its own
// mode (bits_complement).  The set's ITEMS are every wanted member of every part (sign + in
// direct mode, - in complement mode) and every complement part's stored sum (sign +): the
// aggregate is the signed sum of the items, no final subtraction.
//
// n_bits bits of src from bit bit_off on, as the words of a staged field (tail of the last
// word zeroed, as bits_stage leaves it); src is read up to the byte of bit bit_off + n_bits - 1
inline void bits_stage_shifted(uint32_t* dst, const uint8_t* src, uint64_t bit_off, uint32_t n_bits) {
  const size_t nw = bits_words(n_bits);
  const uint8_t* b = src + (bit_off >> 3);
  const unsigned sh = (unsigned)(bit_off & 7);
  const size_t nb = ((size_t)sh + n_bits + 7) >> 3;  // source bytes holding the run
  for (size_t w = 0; w < nw; w++) {
    uint64_t v = 0;  // the 5 bytes from 4 w on: 32 bits after any shift below 8
    for (size_t k = 0; k < 5 && 4 * w + k < nb; k++) v |= (uint64_t)b[4 * w + k] << (8 * k);
    dst[w] = (uint32_t)(v >> sh);
  }
  if (n_bits & 31) dst[nw - 1] &= (1u << (n_bits & 31)) - 1u;
}
// participants among the n_bits bits of src from bit bit_off on
inline uint32_t bits_count_range(const uint8_t* src, uint64_t bit_off, uint32_t n_bits) {
  uint32_t p = 0;
  uint64_t k = bit_off;
  const uint64_t end = bit_off + n_bits;
  for (; k < end && (k & 7); k++) p += (src[k >> 3] >> (k & 7)) & 1u;
  for (; k + 8 <= end; k += 8) p += (uint32_t)__builtin_popcount(src[k >> 3]);
  for (; k < end; k++) p += (src[k >> 3] >> (k & 7)) & 1u;
  return p;
}

struct MultiPart {
  uint32_t committee = 0;
  uint32_t word_off = 0;  // its field's first word in the bit arena
  uint32_t n_bits = 0;
  uint32_t p = 0;         // participants
};
// One multi set as staged: n_parts == 0 means "write the identity" (a set whose error the host
// already knows, or with no participant).  items: wanted members + complement parts' sums.
struct MultiSet {
  uint32_t first_part = 0, n_parts = 0;
  uint32_t p = 0;      // participants over all parts
  uint32_t items = 0;
  int32_t out = 0;     // aggregate slot (the set's staging position)
};
// A set of k registered committees (ids, their lengths lens: n_bits == their sum) as the stager
// records it: the parts with an item appended to `parts`, their fields to the arena (*words in
// use; at most ceil(n_bits / 32) + k words).  A part without a participant has no item and is
// left out; with no participant at all the set is the identity entry and nothing is staged.
inline MultiSet multi_stage_set(const uint32_t* ids, const uint32_t* lens, uint32_t k, const uint8_t* bits,
                                uint32_t n_bits, int32_t out, uint32_t* arena, size_t* words,
                                std::vector<MultiPart>& parts) {
  MultiSet m;
  m.out = out;
  m.first_part = (uint32_t)parts.size();
  if (!bits_count(bits, n_bits)) return m;
  uint64_t off = 0;
  for (uint32_t c = 0; c < k; off += lens[c], c++) {
    MultiPart q;
    q.p = bits_count_range(bits, off, lens[c]);
    if (!q.p) continue;
    q.committee = ids[c];
    q.word_off = (uint32_t)*words;
    q.n_bits = lens[c];
    bits_stage_shifted(arena + *words, bits, off, lens[c]);
    *words += bits_words(lens[c]);
    parts.push_back(q);
    m.n_parts++;
    m.p += q.p;
    m.items += bits_wanted(q.n_bits, q.p) + (bits_complement(q.n_bits, q.p) ? 1u : 0u);
  }
  return m;
}
// Plan of k_pk_agg_bits_multi (words: lsg_bits.h).  A set gets 2^l lane pairs from its item
// count by the rule of bits_pairs_log2 -- at most one wave's 32 pairs, the serial fold grows
// beyond -- and the sets are laid out widest first, so a set starts on a multiple of its width
// and never straddles a wave.  While the launch is work-bound the fold doubles, as in plan_bits.
constexpr int MULTI_SET_WORDS = LSG_MULTI_SET_WORDS;
constexpr int MULTI_PART_WORDS = LSG_MULTI_PART_WORDS;
struct MultiPlan {
  size_t n_sets = 0, n_pairs = 0;
  int fold = BITS_FOLD;
  size_t set_off = 0;   // n_sets x MULTI_SET_WORDS words in the arena
  size_t part_off = 0;  // every part x MULTI_PART_WORDS words
  size_t pair_off = 0;  // n_pairs words: the plan entry each lane pair works for
};
inline MultiPlan plan_multi(std::vector<int32_t>& A, const std::vector<MultiSet>& sets,
                            const std::vector<MultiPart>& parts) {
  MultiPlan P;
  P.n_sets = sets.size();
  if (sets.empty()) return P;
  std::vector<uint32_t> order(sets.size());
  std::vector<int> lg(sets.size());
  for (;; P.fold *= 2) {
    size_t pairs = 0;
    for (size_t i = 0; i < sets.size(); i++) {
      order[i] = (uint32_t)i;
      lg[i] = sets[i].n_parts ? bits_pairs_log2(sets[i].items, P.fold) : 0;
      pairs += (size_t)1 << lg[i];
    }
    if (pairs <= BITS_WIDE_PAIRS || P.fold >= BITS_FOLD_WIDE) break;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lg[a] > lg[b]; });
  P.set_off = A.size();
  size_t pair = 0;
  for (uint32_t i : order) {
    const MultiSet& m = sets[i];
    A.push_back((int32_t)m.first_part);
    A.push_back((int32_t)m.n_parts);
    A.push_back(m.out);
    A.push_back(lg[i]);
    A.push_back((int32_t)pair);
    pair += (size_t)1 << lg[i];
  }
  P.n_pairs = pair;
  P.part_off = A.size();
  for (const MultiPart& q : parts) {
    A.push_back((int32_t)q.committee);
    A.push_back((int32_t)q.word_off);
    A.push_back((int32_t)q.n_bits);
    A.push_back(bits_complement(q.n_bits, q.p) ? 1 : 0);
  }
  P.pair_off = A.size();
  for (size_t e = 0; e < order.size(); e++) A.insert(A.end(), (size_t)1 << lg[order[e]], (int32_t)e);
  return P;
}

// ---- phase-A groups
// What a phase-A group answers for: the package's batchable sets, one 16-job chunk, one
// sub-package of a coalesced launch, one non-batchable job, or every non-batchable job.
struct Owner {
  enum Kind { package, chunk, sub_package, job, nb_merged };
  Kind kind = package;
  size_t index = 0;  // the chunk, sub-package or job
};

struct GroupPlan {
  std::vector<Grp> groups;   // MSM groups first
  std::vector<Owner> owner;  // per group
  // per group, the set sub-ranges its Miller items must not cross (PhasePlan::sub): the 16-job
  // chunks of a package group, so that a failing group's chunks (phase B) reuse its items; the
  // jobs of the merged non-batchable group
  std::vector<std::vector<Range>> sub;
  // per set: alone in its phase-A group (and so in every later one), verified unscaled (r_i = 0)
  std::vector<uint8_t> noscale;
  bool lone_unscaled = false;  // ... and that group is the package group
  int big_g = -1;              // the package group (-1: none)
  int nb_g = -1;               // the merged non-batchable group (-1: one group per job)
  bool chunk_mode = false;     // one group per 16-job chunk instead of package groups
  std::vector<int> chunk_group;  // chunk mode: per chunk, its group (-1: no sets)
  std::vector<int> sub_big;      // a coalesced launch: per sub-package, its package group (-1: none)
  std::vector<int> job_group;    // per job: its phase-A group (non-batchable with sets), else -1
  // after plan_phase (group_items): per chunk its items in its package group, per job its items
  // in the merged non-batchable group; (-1, -1): none
  std::vector<ItemRange> chunk_items, nb_items;
};

// chunks (indices into `chunks`) with sets that group owner `o` covers, in order
inline std::vector<size_t> owner_chunks(const PkgShape& sh, const std::vector<Range>& chunks, const Owner& o) {
  std::vector<size_t> out;
  if (o.kind != Owner::package && o.kind != Owner::sub_package) return out;
  Range pos = {0, sh.batch_order.size()};  // the owner's batch_order positions; chunks are in position order
  if (o.kind == Owner::sub_package) pos = {sh.bpos_first[o.index], sh.bpos_first[o.index + 1]};
  size_t c = (size_t)(std::lower_bound(chunks.begin(), chunks.end(), Range(pos.first, 0)) - chunks.begin());
  for (; c < chunks.size() && chunks[c].first < pos.second; c++)
    if (pos_sets(sh, chunks[c]).len) out.push_back(c);
  return out;
}

// Phase A: one RLC group per package (a coalesced launch: per sub-package; chunk mode: per
// 16-job chunk), one per non-batchable job or one for all of them.
// lone_ok: a set alone in its group may be verified unscaled (a plain verify, as
// maybeBatch.ts:34-38).  False when the package group's partial is multiplied with other
// partials before its verdict: there every r_i is random and nonzero.
inline GroupPlan plan_groups(const PkgShape& sh, const Switches& sw, bool lone_ok) {
  GroupPlan gp;
  const size_t nj = sh.jobs.size();
  const bool subs = sh.n_sub > 0;
  const bool per_sub = sw.package_group && subs && sw.sub_groups;
  gp.chunk_mode = !sw.package_group || (subs && !sw.sub_groups);
  const std::vector<Range> chunks = pkg_chunks(sh);
  // the merged non-batchable group: every one of its sets is randomised, so a one-set job in
  // it is scaled too (its own check, if the group fails, stays exact: r_i != 0)
  std::vector<size_t> nonb;  // non-batchable jobs with sets
  for (size_t k = 0; k < nj; k++)
    if (!batchable(sh.jobs[k]) && sh.jobs[k].count) nonb.push_back(k);
  const bool nb_merge = sw.nb_merge && nonb.size() >= 2 && !subs && sw.package_group;

  struct Item {
    Grp g;
    Owner o;
  };
  std::vector<Item> items;
  auto add = [&](Grp g, Owner::Kind kind, size_t index) {
    if (!g.len) return;
    g.msm = g.len >= std::max(sw.msm_min_group, (size_t)2);  // an r_i = 0 set never enters a bucket MSM
    Owner o;
    o.kind = kind;
    o.index = index;
    items.push_back({g, o});
  };
  if (gp.chunk_mode) {
    for (size_t c = 0; c < chunks.size(); c++) add(pos_sets(sh, chunks[c]), Owner::chunk, c);
  } else if (subs) {
    for (size_t k = 0; k < (size_t)sh.n_sub; k++)
      add(pos_sets(sh, {sh.bpos_first[k], sh.bpos_first[k + 1]}), Owner::sub_package, k);
  } else {
    add(pos_sets(sh, {0, sh.batch_order.size()}), Owner::package, 0);
  }
  if (nb_merge) {  // staged contiguously after the batchable sets, in job order
    Grp g = job_sets(sh.jobs[nonb.front()]);
    g.len = sh.jobs[nonb.back()].first + sh.jobs[nonb.back()].count - g.first;
    add(g, Owner::nb_merged, 0);
  } else {
    for (size_t k : nonb) add(job_sets(sh.jobs[k]), Owner::job, k);
  }
  std::stable_partition(items.begin(), items.end(), [](const Item& x) { return x.g.msm; });

  const size_t ng = items.size();
  gp.chunk_group.assign(gp.chunk_mode ? chunks.size() : 0, -1);
  gp.sub_big.assign((size_t)sh.n_sub, -1);
  gp.job_group.assign(nj, -1);
  const bool pkg_sub = !gp.chunk_mode && sh.nb_sets;
  if (nb_merge || pkg_sub) gp.sub.assign(ng, {});
  for (size_t g = 0; g < ng; g++) {
    gp.groups.push_back(items[g].g);
    gp.owner.push_back(items[g].o);
    const Owner& o = items[g].o;
    switch (o.kind) {
      case Owner::package: gp.big_g = (int)g; break;
      case Owner::chunk: gp.chunk_group[o.index] = (int)g; break;
      case Owner::sub_package: gp.sub_big[o.index] = (int)g; break;
      case Owner::job: gp.job_group[o.index] = (int)g; break;
      case Owner::nb_merged:
        gp.nb_g = (int)g;
        for (size_t k : nonb) {  // the merged group's items never cross a job
          gp.job_group[k] = (int)g;
          gp.sub[g].push_back({sh.jobs[k].first, sh.jobs[k].first + sh.jobs[k].count});
        }
        break;
    }
    // a package group's items never cross a 16-job chunk
    if (pkg_sub)
      for (size_t c : owner_chunks(sh, chunks, o)) {
        const Grp cs = pos_sets(sh, chunks[c]);
        gp.sub[g].push_back({cs.first, cs.first + cs.len});
      }
  }

  size_t n_sets = 0;
  for (const JobRec& J : sh.jobs) n_sets += J.count;
  gp.noscale.assign(n_sets, 0);
  if (lone_ok) {  // (non-batchable jobs below: their groups never enter the package partial)
    std::vector<Grp> lone;
    if (gp.chunk_mode) {
      for (auto& c : chunks) lone.push_back(pos_sets(sh, c));
    } else if (per_sub) {
      for (size_t k = 0; k < (size_t)sh.n_sub; k++) lone.push_back(pos_sets(sh, {sh.bpos_first[k], sh.bpos_first[k + 1]}));
    } else {
      gp.lone_unscaled = sh.nb_sets == 1;
      lone.push_back(pos_sets(sh, {0, sh.batch_order.size()}));
    }
    for (const Grp& g : lone)
      if (g.len == 1) gp.noscale[g.first] = 1;
  }
  if (!nb_merge)
    for (size_t k : nonb)
      if (sh.jobs[k].count == 1) gp.noscale[sh.jobs[k].first] = 1;
  return gp;
}

// After plan_phase(A) of the plan's groups: the items of every chunk within its package group
// and of every job within the merged non-batchable group, from A.sub_items.
inline void group_items(GroupPlan& gp, const PkgShape& sh, const PhasePlan& A) {
  const std::vector<Range> chunks = pkg_chunks(sh);
  gp.chunk_items.assign(chunks.size(), {-1, -1});
  gp.nb_items.assign(gp.nb_g >= 0 ? sh.jobs.size() : 0, {-1, -1});
  size_t r = 0;
  for (size_t g = 0; g < gp.groups.size(); g++) {
    if ((int)g == A.agg_g) continue;  // (message items: no sub_items entries)
    const size_t ns = g < gp.sub.size() && !gp.sub[g].empty() ? gp.sub[g].size() : 1;
    if ((int)g == gp.nb_g) {
      size_t q = r;
      for (size_t k = 0; k < sh.jobs.size(); k++)
        if (gp.job_group[k] == gp.nb_g) gp.nb_items[k] = A.sub_items[q++];
    } else {
      size_t q = r;
      for (size_t c : owner_chunks(sh, chunks, gp.owner[g])) gp.chunk_items[c] = A.sub_items[q++];
    }
    r += ns;
  }
}

// ---- the verdict rules
// check(groups, given, verdicts): one fallback phase -- verdicts[g] = 1 iff the RLC check of
// groups[g] passes (sets with an error are the identity in it).  given (or null): per group,
// its items among phase A's resident Miller items.  Returns LSG_OK or an error to pass on.
typedef std::function<int(const std::vector<Grp>&, const std::vector<ItemRange>*, std::vector<int32_t>&)> CheckFn;

// what resolve_package writes: per-job results, the package's counters and, for a coalesced
// launch, every sub-package's counters and bad-key code
struct PkgVerdicts {
  std::vector<lsg_job_result>& results;
  lsg_stats& stats;
  std::vector<lsg_stats>& sub_stats;
  std::vector<int32_t>& sub_pkfail;
};

// The reference's verdict rules for one device's share of a package (worker.ts:30-106).
//   vA: the phase-A groups' verdicts (a deferred package-group verdict already settled)
//   pkfail: the package-wide deserializeSet failure (first_key_error over every device of the
//     ticket, in caller order) -- a bad key on any device rejects every job of the package
//   it_first / it_cnt: phase A's Miller items (PhasePlan)
struct Resolver {
  const PkgShape& sh;
  const GroupPlan& gp;
  const SetStatus& ss;
  const std::vector<int32_t>& vA;
  const std::vector<int32_t>&it_first, &it_cnt;
  const Switches& sw;
  const CheckFn& check;
  PkgVerdicts out;

  // a chunk of a failing package group, to be checked on its own (phase B)
  struct ChunkCheck {
    Grp sets;
    Range jobs;       // batch_order positions
    ItemRange items;  // its resident phase-A items
    bool threw;       // the chunk threw (its retry is counted already, no batch success)
  };
  std::vector<uint8_t> job_dead;  // the job's sub-package has a bad key
  std::vector<uint8_t> job_err;   // the job's result is its decode error
  std::vector<ChunkCheck> chk;
  std::vector<size_t> fail_chunks;  // phase-B chunks that failed, whose phase-A items phase C1 reuses
  std::vector<size_t> retry;        // jobs verified individually (phase C2)

  const JobRec& job_at(size_t q) const { return sh.jobs[sh.batch_order[q]]; }
  // counters of the chunk at batch_order position q: the package's, and its sub-package's
  void retry_inc(size_t q) {
    out.stats.batch_retries++;
    if (sh.n_sub) out.sub_stats[(size_t)sub_of_pos(sh, q)].batch_retries++;
  }
  void succ_add(size_t q, size_t len) {
    out.stats.batch_sigs_success += (uint32_t)len;
    if (sh.n_sub) out.sub_stats[(size_t)sub_of_pos(sh, q)].batch_sigs_success += (uint32_t)len;
  }
  // every job at positions r that did not throw: one verdict / verified on its own
  void answer_live(Range r, lsg_job_result v) {
    for (size_t q = r.first; q < r.second; q++)
      if (!job_err[sh.batch_order[q]]) out.results[sh.batch_order[q]] = v;
  }
  void retry_live(Range r) {
    for (size_t q = r.first; q < r.second; q++)
      if (!job_err[sh.batch_order[q]]) retry.push_back(sh.batch_order[q]);
  }

  // a coalesced launch: the deserializeSet rule per sub-package (worker.ts:41-43)
  void sub_package_keys() {
    for (size_t k = 0; k < (size_t)sh.n_sub; k++) {
      size_t ej = 0;
      const int32_t e = first_key_error(sh, ss.pkerr, sh.sub_first[k], sh.sub_first[k + 1], &ej);
      out.sub_pkfail[k] = e;
      out.sub_stats[k].key_error = e;
      out.sub_stats[k].key_error_job = e ? (uint32_t)(ej - sh.sub_first[k]) : 0;
      if (e)
        for (size_t j = sh.sub_first[k]; j < sh.sub_first[k + 1]; j++) {
          out.results[j] = {LSG_ERROR, e};
          job_dead[j] = 1;
        }
    }
  }

  // non-batchable jobs: their own group (worker.ts:88-96), or the merged group (nb_g): a
  // passing one answers every such job; a failing one is localised job by job over the jobs'
  // resident phase-A items (a fallback phase), so each verdict is still the job's own
  int non_batchable() {
    std::vector<Grp> nbg;
    std::vector<size_t> nbj;
    std::vector<ItemRange> nbi;
    for (size_t j = 0; j < sh.jobs.size(); j++) {
      if (batchable(sh.jobs[j]) || job_dead[j]) continue;
      const int g = gp.job_group[j];
      const int32_t e = job_error(ss, sh.jobs[j].first, sh.jobs[j].count);  // (no sets: maybeBatch.ts:29-31)
      if (!e && g == gp.nb_g && !vA[(size_t)g]) {
        nbg.push_back(job_sets(sh.jobs[j]));
        nbj.push_back(j);
        nbi.push_back(gp.nb_items[j]);
        continue;
      }
      out.results[j] = e ? lsg_job_result{LSG_ERROR, e} : lsg_job_result{vA[(size_t)g] ? LSG_VALID : LSG_INVALID, 0};
    }
    if (nbg.empty()) return LSG_OK;
    std::vector<int32_t> vn;
    if (const int rc = check(nbg, &nbi, vn)) return rc;
    for (size_t k = 0; k < nbj.size(); k++) out.results[nbj[k]] = {vn[k] ? LSG_VALID : LSG_INVALID, 0};
    return LSG_OK;
  }

  // batchable jobs: chunks of >= 16 jobs (worker.ts:51-86), each answered by the phase-A group
  // that covers it, sent to phase B (chk) or to the per-job phase (retry)
  void classify_chunks() {
    const std::vector<Range> chunks = pkg_chunks(sh);
    std::vector<uint8_t> chunk_err(chunks.size(), 0);
    bool any_err_chunk = false;
    for (size_t c = 0; c < chunks.size(); c++) {
      const Grp cs = pos_sets(sh, chunks[c]);
      for (size_t i = cs.first; i < cs.first + cs.len && !chunk_err[c]; i++) chunk_err[c] = set_error(ss, i) != 0;
      any_err_chunk = any_err_chunk || chunk_err[c];
    }
    // the package group covering chunk c passed (a coalesced launch: its sub-package's group)
    auto pkg_ok = [&](size_t c) {
      const int g = sh.n_sub ? gp.sub_big[(size_t)sub_of_pos(sh, chunks[c].first)] : gp.big_g;
      return g < 0 || vA[(size_t)g] != 0;
    };
    // the package group is exactly chunk c (a coalesced sub-package of exactly one chunk: its
    // group has the chunk's sets and r_i): its verdict is the chunk's
    std::vector<int> sub_nchunks((size_t)sh.n_sub, 0);
    for (size_t c = 0; c < chunks.size() && sh.n_sub; c++) sub_nchunks[(size_t)sub_of_pos(sh, chunks[c].first)]++;
    auto group_is_chunk = [&](size_t c) {
      if (!sh.n_sub) return chunks.size() == 1 && !any_err_chunk;
      return sub_nchunks[(size_t)sub_of_pos(sh, chunks[c].first)] == 1;  // (chunk c has no decode error)
    };
    for (size_t c = 0; c < chunks.size(); c++) {
      const Range r = chunks[c];
      if (job_dead[sh.batch_order[r.first]]) continue;  // its sub-package has a bad key
      const Grp cs = pos_sets(sh, r);
      if (cs.len == 0) {  // maybeBatch([]) throws: retried, and every job throws again
        retry_inc(r.first);
        answer_live(r, {LSG_ERROR, LSG_ERR_EMPTY_SET});
        continue;
      }
      const bool threw = chunk_err[c] != 0;
      if (threw) {  // worker.ts:79-85: every job is verified on its own
        retry_inc(r.first);
        // A job's own verdict is its validity alone, so the chunk's jobs that do not throw are
        // checked as ONE group first -- the throwing sets are the identity in the chunk's items
        // and signature sums (the kernels' err rule) -- and localised only if it fails: a chunk
        // with one undecodable signature costs one group check instead of 16 per-job checks.
        // Verdicts and the batch counters are the reference's (the retry counted above, no
        // batch success for a chunk that threw).
        bool live = false;
        for (size_t q = r.first; q < r.second; q++) {
          const size_t j = sh.batch_order[q];
          const int32_t e = job_error(ss, sh.jobs[j].first, sh.jobs[j].count);
          if (e) {
            out.results[j] = {LSG_ERROR, e};
            job_err[j] = 1;
          } else {
            live = true;
          }
        }
        if (!live) continue;
      }
      // chunk mode: the chunk's own phase-A group decides; else the package group covering it
      const bool is_chunk = gp.chunk_mode || (!threw && group_is_chunk(c));
      const bool ok = gp.chunk_mode ? vA[(size_t)gp.chunk_group[c]] != 0 : pkg_ok(c);
      if (ok) {
        answer_live(r, {LSG_VALID, 0});
        if (!threw) succ_add(r.first, cs.len);
      } else if (is_chunk) {
        if (!threw) retry_inc(r.first);
        retry_live(r);
      } else {
        chk.push_back({cs, r, gp.chunk_items[c], threw});
      }
    }
  }

  // Phases B0 and B: the chunks of a failing package group, each checked on its own.
  int check_chunks() {
    if (chk.empty()) return LSG_OK;
    bool reuse = true;
    for (auto& c : chk) reuse = reuse && c.items.first >= 0;
    // Phase B0: runs of consecutive chunks (adjacent sets and resident items) as one group
    // each, so that only the chunks of a failing run are checked on their own.  A run passes
    // only if every chunk in it would (the RLC check of its sets, the throwing sets the
    // identity as in the chunks' own groups), so each chunk's verdict -- and with it the batch
    // counters below -- is what its own check gives.  At 1 % corrupted sets about a fifth of
    // the runs of four fail: 2048 chunk checks of a 32k package become ~512 + ~460.
    std::vector<uint8_t> passed(chk.size(), 0);
    if (reuse && sw.b0_min > 0 && chk.size() >= sw.b0_min) {
      std::vector<Grp> rg;
      std::vector<ItemRange> ri;
      std::vector<Range> rc;  // chk index range [a, b) of each run
      for (size_t c = 0; c < chk.size();) {
        size_t e = c + 1;
        while (e < chk.size() && e - c < sw.b0_run && chk[e].sets.first == chk[e - 1].sets.first + chk[e - 1].sets.len &&
               chk[e].items.first == chk[e - 1].items.second)
          e++;
        if (e - c >= 2) {
          Grp g;
          g.first = chk[c].sets.first;
          g.len = chk[e - 1].sets.first + chk[e - 1].sets.len - chk[c].sets.first;
          rg.push_back(g);
          ri.push_back({chk[c].items.first, chk[e - 1].items.second});
          rc.push_back({c, e});
        }
        c = e;
      }
      if (!rg.empty()) {
        std::vector<int32_t> vr;
        if (const int rcode = check(rg, &ri, vr)) return rcode;
        for (size_t k = 0; k < rg.size(); k++)
          if (vr[k])
            for (size_t c = rc[k].first; c < rc[k].second; c++) passed[c] = 1;
      }
    }
    // Phase B: the chunks no passing run answered
    std::vector<Grp> rest;
    std::vector<ItemRange> rest_items;
    std::vector<size_t> rest_of;
    for (size_t c = 0; c < chk.size(); c++)
      if (!passed[c]) {
        rest.push_back(chk[c].sets);
        rest_items.push_back(chk[c].items);
        rest_of.push_back(c);
      }
    std::vector<int32_t> vb;
    if (const int rcode = check(rest, reuse ? &rest_items : nullptr, vb)) return rcode;
    for (size_t k = 0; k < rest.size(); k++) passed[rest_of[k]] = vb[k] != 0;
    for (size_t c = 0; c < chk.size(); c++) {
      if (passed[c]) {
        answer_live(chk[c].jobs, {LSG_VALID, 0});
        if (!chk[c].threw) succ_add(chk[c].jobs.first, chk[c].sets.len);
      } else {
        if (!chk[c].threw) retry_inc(chk[c].jobs.first);
        if (reuse)
          fail_chunks.push_back(c);
        else
          retry_live(chk[c].jobs);
      }
    }
    return LSG_OK;
  }

  // Phase C1: the jobs of a failing chunk, localised over its phase-A items.  A group is a
  // run of whole items ending on a job boundary (for single-set jobs: one item = four jobs),
  // checked with its resident items -- no new Miller work.  A passing group answers its jobs
  // (valid); a one-job group's verdict is that job's maybeBatch verdict (the same RLC check,
  // worker.ts:88-96); the jobs of a failing multi-job group are checked one by one (C2).
  // Per-job verdicts and the batch counters are unchanged: only the work is (a chunk with one
  // bad set costs 4 group checks + 4 one-set checks instead of 16 one-set checks).
  int localise_items() {
    if (fail_chunks.empty()) return LSG_OK;
    std::vector<Grp> g1;
    std::vector<ItemRange> g1_items;
    std::vector<Range> g1_jobs;  // batch_order positions [a, b)
    for (size_t c : fail_chunks) {
      size_t q = chk[c].jobs.first;
      const size_t qe = chk[c].jobs.second;
      // a job without sets throws when it is retried (maybeBatch.ts:29-31), whatever the group
      // its position falls into says
      for (size_t p = q; p < qe; p++)
        if (job_at(p).count == 0) {
          out.results[sh.batch_order[p]] = {LSG_ERROR, LSG_ERR_EMPTY_SET};
          job_err[sh.batch_order[p]] = 1;
        }
      const ItemRange items = chk[c].items;
      int32_t ia = items.first;
      for (int32_t it = items.first; it < items.second; it++) {
        const size_t end = (size_t)it_first[(size_t)it] + (size_t)it_cnt[(size_t)it];
        // jobs of this group: those ending at or before `end`; close the group on a boundary
        size_t qb = q;
        while (qb < qe && job_at(qb).first + job_at(qb).count <= end) qb++;
        const bool boundary = qb > q && job_at(qb - 1).first + job_at(qb - 1).count == end;
        if (!boundary && it + 1 < items.second) continue;
        Grp g;
        g.first = (size_t)it_first[(size_t)ia];
        g.len = end - g.first;
        g1.push_back(g);
        g1_items.push_back({ia, it + 1});
        g1_jobs.push_back({q, qb});
        q = qb;
        ia = it + 1;
      }
      for (; q < qe; q++) retry.push_back(sh.batch_order[q]);  // (not reached: items cover the chunk)
    }
    std::vector<int32_t> v;
    if (const int rc = check(g1, &g1_items, v)) return rc;
    for (size_t g = 0; g < g1.size(); g++) {
      // A thrown job keeps its error.  Only its throwing sets are the identity in the group:
      // its other sets take part, so a failing group with one live job localises that job on
      // its own (C2) unless every other job of the group is live too.
      size_t nlive = 0;
      for (size_t q = g1_jobs[g].first; q < g1_jobs[g].second; q++) nlive += job_err[sh.batch_order[q]] ? 0 : 1;
      const bool thrown = nlive < g1_jobs[g].second - g1_jobs[g].first;
      if (v[g])
        answer_live(g1_jobs[g], {LSG_VALID, 0});
      else if (nlive == 1 && !thrown)
        answer_live(g1_jobs[g], {LSG_INVALID, 0});
      else
        retry_live(g1_jobs[g]);
    }
    return LSG_OK;
  }

  // Phase C2: one group per job (worker.ts:88-96)
  int check_jobs() {
    if (retry.empty()) return LSG_OK;
    std::vector<Grp> g3;
    std::vector<size_t> g3job;
    for (size_t j : retry) {
      const int32_t e = job_error(ss, sh.jobs[j].first, sh.jobs[j].count);
      if (e) {
        out.results[j] = {LSG_ERROR, e};
        continue;
      }
      g3.push_back(job_sets(sh.jobs[j]));
      g3job.push_back(j);
    }
    std::vector<int32_t> v;
    if (const int rc = check(g3, nullptr, v)) return rc;
    for (size_t g = 0; g < g3.size(); g++) out.results[g3job[g]] = {v[g] ? LSG_VALID : LSG_INVALID, 0};
    return LSG_OK;
  }

  int run(int32_t pkfail) {
    const size_t nj = sh.jobs.size();
    if (pkfail) {
      for (size_t j = 0; j < nj; j++) out.results[j] = {LSG_ERROR, pkfail};
      return LSG_OK;
    }
    job_dead.assign(nj, 0);
    job_err.assign(nj, 0);
    sub_package_keys();
    if (const int rc = non_batchable()) return rc;
    if (sh.batch_order.empty()) return LSG_OK;
    // The device's own check of its share (computed in phase A in any case) decides.  The
    // node-wide verdict is advisory: a passing node check with a failing own check (a caller
    // whose all-gather missed a rank) localises like a failing one instead of
    // accepting the package.
    classify_chunks();
    if (const int rc = check_chunks()) return rc;
    if (const int rc = localise_items()) return rc;
    return check_jobs();
  }
};

inline int resolve_package(const PkgShape& sh, const GroupPlan& gp, const SetStatus& ss, const std::vector<int32_t>& vA,
                           int32_t pkfail, const PhasePlan& phA, const Switches& sw, const CheckFn& check,
                           PkgVerdicts out) {
  Resolver r{sh, gp, ss, vA, phA.it_first, phA.it_cnt, sw, check, out};
  return r.run(pkfail);
}

// ---- per-group sums of the verified signatures (lsg_submit_jobs_grouped)
// The staged sets whose signature joins its group's aggregate: set i of job k (staging order,
// verdicts[k] that job's) is included exactly when the job resolved to LSG_VALID -- a multi-set
// job all or nothing, as its verdict is.
inline std::vector<uint8_t> included_sets(const PkgShape& sh, const lsg_job_result* verdicts) {
  size_t n = 0;
  for (const JobRec& J : sh.jobs) n = std::max(n, J.first + J.count);
  std::vector<uint8_t> mask(n, 0);
  for (size_t k = 0; k < sh.jobs.size(); k++)
    if (verdicts[k].status == LSG_VALID)
      for (size_t i = sh.jobs[k].first; i < sh.jobs[k].first + sh.jobs[k].count; i++) mask[i] = 1;
  return mask;
}

// The plan of k_sig_agg_seg (lsg_k_sig.hip) appended to arena A.  set_group[i] is staged set i's
// group (below n_groups, or LSG_NO_GROUP); mask (null: every set) leaves out the sets with
// mask[i] == 0.  gather: n_gather words at A[gather_off ..] holding the n_members set slots
// ordered by group and within a group by slot; group g's members are gather[off[g] .. off[g] +
// len[g]).  seg: plan_seg over that list (its first pass is the kernel's, reading sets through
// the list; a group longer than one chunk of 2^ips_log2 lane pairs x SEG_FOLD members finishes
// in a second pass of k_seg_reduce<1> over the chunk sums).  An empty group keeps a chunk of
// length 0: the identity.
// A group of SIG_GROUP_PAD_MIN members or more is followed by SIG_GROUP_PAD unused words (one
// cache line): packed back to back, groups of one power-of-two length (64 committees of 512)
// start at one power-of-two stride, and the write streams of the fill below then evict one
// another from the same few cache sets (the fill of 32,768 sets took six times as long).
constexpr int32_t SIG_GROUP_PAD_MIN = 128, SIG_GROUP_PAD = 16;
struct SigGroupPlan {
  size_t gather_off = 0, n_gather = 0, n_members = 0;
  std::vector<int32_t> off, len;  // per group
  SegPlan seg;
};
inline SigGroupPlan plan_sig_groups(std::vector<int32_t>& A, const uint32_t* set_group, size_t n_sets, size_t n_groups,
                                    const uint8_t* mask, int fold_wide = SEG_FOLD_WIDE) {
  SigGroupPlan P;
  P.off.assign(n_groups, 0);
  P.len.assign(n_groups, 0);
  auto in = [&](size_t i) { return set_group[i] < n_groups && (!mask || mask[i]); };
  for (size_t i = 0; i < n_sets; i++)
    if (in(i)) P.len[set_group[i]]++;
  int32_t tot = 0;
  for (size_t g = 0; g < n_groups; g++) {
    P.off[g] = tot;
    P.n_members += (size_t)P.len[g];
    tot += P.len[g] + (P.len[g] >= SIG_GROUP_PAD_MIN ? SIG_GROUP_PAD : 0);
  }
  P.gather_off = A.size();
  P.n_gather = (size_t)tot;
  A.resize(P.gather_off + P.n_gather);
  std::vector<int32_t> fill(P.off);
  for (size_t i = 0; i < n_sets; i++)
    if (in(i)) A[P.gather_off + (size_t)fill[set_group[i]]++] = (int32_t)i;
  P.seg = plan_seg(A, 1, P.off, P.len, true, P.gather_off, 0, fold_wide);
  return P;
}

}  // namespace lsgp
