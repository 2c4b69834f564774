// groupcheck.cpp -- CPU driver of the signature-group policy in lodestar_amd/csrc/lsg_plan.hpp
// (tests/test_sig_groups_host.py): included_sets and plan_sig_groups.  No device: a set's
// signature is an integer mod the prime 2^61 - 1, "addition" is addition mod that prime, the
// identity is 0.  A case's plan is executed as the device executes it: the first pass as
// k_sig_agg_seg does (lane pair j of a chunk folds list entries j, j + ips, ... through the
// gather list, then the butterfly over the chunk's pairs within its wave), later passes as
// k_seg_reduce<1> does over the chunk sums.
//
//   groupcheck CASES OUT    CASES: whitespace-separated integers, OUT: one line per case
//
// CASES = n_cases, then per case its kind:
//   0 (groups)   n_sets n_groups has_mask, per set: group (-1: LSG_NO_GROUP) value mask
//   1 (included) n_jobs, per job: n_sets flags status
// OUT per case:
//   kind 0: per group "sum len", then "P n_members n_passes ips_log2 cap tmp_items" (first pass)
//   kind 1: per job (caller order) "first count", then "M" and the mask, one digit per staged set
// Any broken invariant prints a message and exits nonzero.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <string>

#include "../../lodestar_amd/csrc/lsg_plan.hpp"

using namespace lsgp;

namespace {

constexpr uint64_t PRIME = (1ull << 61) - 1;

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "groupcheck: %s\n", m.c_str());
  exit(2);
}
#define REQUIRE(c, m) \
  do {                \
    if (!(c)) die(m); \
  } while (0)

struct Input {
  std::vector<long long> v;
  size_t at = 0;
  long long next() {
    REQUIRE(at < v.size(), "case file ends early");
    return v[at++];
  }
};

uint64_t add(uint64_t a, uint64_t b) { return (a + b) % PRIME; }

// One pass of the segmented reduction over `n_chunks` chunks of 2^ips_log2 lane pairs each,
// waves of 32 pairs.  elem(k): element k of the pass's input (k indexes the gather list in the
// first pass, the previous pass's chunk sums later).
template <class Elem>
void run_pass(const int32_t* chunks, int n_chunks, int ips_log2, size_t n_in, Elem elem, std::vector<uint64_t>& dst,
              std::vector<uint8_t>& dst_set, std::vector<uint64_t>& tmp, std::vector<uint8_t>& tmp_set,
              std::vector<uint32_t>& taken) {
  REQUIRE(ips_log2 >= 0 && ips_log2 <= 5, "a chunk holds more lane pairs than a wave");
  const int ips = 1 << ips_log2;
  const size_t items = (size_t)n_chunks << ips_log2;
  for (size_t w0 = 0; w0 < items; w0 += 32) {
    uint64_t acc[32];
    long long chunk_of[32];
    for (int l = 0; l < 32; l++) {
      acc[l] = 0;
      chunk_of[l] = -1;
      const size_t item = w0 + (size_t)l;
      const size_t c = item >> ips_log2;
      if (c >= (size_t)n_chunks) continue;
      chunk_of[l] = (long long)c;
      const int j = (int)(item & (size_t)(ips - 1));
      const int off = chunks[3 * c], len = chunks[3 * c + 1];
      REQUIRE(off >= 0 && len >= 0 && (size_t)off + (size_t)len <= n_in, "chunk outside its input");
      for (int k = j; k < len; k += ips) {
        acc[l] = add(acc[l], elem((size_t)(off + k)));
        taken[(size_t)(off + k)]++;
      }
    }
    for (int o = ips >> 1; o >= 1; o >>= 1) {
      uint64_t t[32];
      for (int l = 0; l < 32; l++) t[l] = acc[l ^ o];
      for (int l = 0; l < 32; l++) {
        REQUIRE(chunk_of[l ^ o] == chunk_of[l], "butterfly partner belongs to another chunk");
        acc[l] = add(acc[l], t[l]);
      }
    }
    for (int l = 0; l < 32; l++) {
      if (chunk_of[l] < 0 || ((w0 + (size_t)l) & (size_t)(ips - 1)) != 0) continue;
      const int out = chunks[3 * (size_t)chunk_of[l] + 2];
      if (out >= 0) {
        REQUIRE((size_t)out < dst.size() && !dst_set[(size_t)out], "group result written twice or out of range");
        dst[(size_t)out] = acc[l];
        dst_set[(size_t)out] = 1;
      } else {
        const size_t t = (size_t)(-out - 1);
        REQUIRE(t < tmp.size() && !tmp_set[t], "chunk sum written twice or outside tmp_items");
        tmp[t] = acc[l];
        tmp_set[t] = 1;
      }
    }
  }
}

std::string run_groups(Input& in) {
  const size_t n_sets = (size_t)in.next(), n_groups = (size_t)in.next();
  const bool has_mask = in.next() != 0;
  std::vector<uint32_t> grp(n_sets);
  std::vector<uint64_t> val(n_sets);
  std::vector<uint8_t> mask(n_sets);
  for (size_t i = 0; i < n_sets; i++) {
    const long long g = in.next();
    grp[i] = g < 0 ? LSG_NO_GROUP : (uint32_t)g;
    val[i] = (uint64_t)in.next() % PRIME;
    mask[i] = in.next() != 0;
  }
  std::vector<int32_t> A;
  A.push_back(12345);  // (the plan does not start at word 0 of its arena)
  const SigGroupPlan P = plan_sig_groups(A, grp.data(), n_sets, n_groups, has_mask ? mask.data() : nullptr);
  REQUIRE(P.off.size() == n_groups && P.len.size() == n_groups, "one offset and length per group");
  REQUIRE(P.gather_off == 1 && P.gather_off + P.n_gather <= A.size(), "gather list outside the arena");
  // the gather list: every unmasked grouped set exactly once, ordered by group
  const int32_t* gather = A.data() + P.gather_off;
  std::vector<uint8_t> seen(n_sets, 0);
  size_t want = 0;
  for (size_t i = 0; i < n_sets; i++) want += grp[i] != LSG_NO_GROUP && (!has_mask || mask[i]);
  REQUIRE(P.n_members == want, "members != unmasked grouped sets");
  // (a long group is followed by a cache line of unused words: SIG_GROUP_PAD)
  REQUIRE(P.n_gather >= want && P.n_gather <= want + (size_t)SIG_GROUP_PAD * (want / (size_t)SIG_GROUP_PAD_MIN), "list length");
  for (size_t g = 0; g < n_groups; g++) {
    REQUIRE(P.off[g] >= 0 && P.len[g] >= 0 && (size_t)P.off[g] + (size_t)P.len[g] <= P.n_gather, "group range");
    REQUIRE(g == 0 || P.off[g] >= P.off[g - 1] + P.len[g - 1], "group ranges overlap");
    for (int32_t k = P.off[g]; k < P.off[g] + P.len[g]; k++) {
      const int32_t i = gather[k];
      REQUIRE(i >= 0 && (size_t)i < n_sets, "gather entry out of range");
      REQUIRE(grp[(size_t)i] == g && (!has_mask || mask[(size_t)i]) && !seen[(size_t)i], "wrong or repeated member");
      seen[(size_t)i] = 1;
    }
  }
  const SegPlan& S = P.seg;
  REQUIRE(S.op == 1 && S.has_idx && S.idx_off == P.gather_off, "a G2 plan over the gather list");
  REQUIRE(n_groups == 0 || !S.passes.empty(), "no pass for a package with groups");
  std::vector<uint64_t> dst(n_groups, ~0ull), tmp[3];
  std::vector<uint8_t> dst_set(n_groups, 0), tmp_set[3];
  for (size_t k = 0; k < S.passes.size(); k++) {
    const SegPass& q = S.passes[k];
    REQUIRE((k == 0) == (q.src == 0) && (q.tmp_out == 1 || q.tmp_out == 2) && q.tmp_out != q.src, "pass buffers");
    REQUIRE(q.chunk_off + 3 * (size_t)q.n_chunks <= A.size(), "chunks outside the arena");
    tmp[q.tmp_out].assign(S.tmp_items, ~0ull);
    tmp_set[q.tmp_out].assign(S.tmp_items, 0);
    const int32_t* chunks = A.data() + q.chunk_off;
    if (k == 0) {
      std::vector<uint32_t> taken(P.n_gather, 0);
      run_pass(chunks, q.n_chunks, q.ips_log2, P.n_gather, [&](size_t e) { return val[(size_t)gather[e]]; }, dst,
               dst_set, tmp[q.tmp_out], tmp_set[q.tmp_out], taken);
      std::vector<uint8_t> is_member(P.n_gather, 0);
      for (size_t g = 0; g < n_groups; g++)
        for (int32_t e = P.off[g]; e < P.off[g] + P.len[g]; e++) is_member[(size_t)e] = 1;
      for (size_t e = 0; e < P.n_gather; e++) REQUIRE(taken[e] == is_member[e], "a member not added exactly once, or a pad word read");
    } else {
      const std::vector<uint64_t>& src = tmp[q.src];
      const std::vector<uint8_t>& src_set = tmp_set[q.src];
      size_t n_in = 0;
      while (n_in < src_set.size() && src_set[n_in]) n_in++;
      std::vector<uint32_t> taken(n_in, 0);
      run_pass(chunks, q.n_chunks, q.ips_log2, n_in, [&](size_t e) { return src[e]; }, dst, dst_set, tmp[q.tmp_out],
               tmp_set[q.tmp_out], taken);
      for (uint32_t t : taken) REQUIRE(t == 1, "a chunk sum not added exactly once");
    }
  }
  std::string line;
  for (size_t g = 0; g < n_groups; g++) {
    REQUIRE(dst_set[g], "a group without a result");
    line += std::to_string(dst[g]) + " " + std::to_string(P.len[g]) + " ";
  }
  const int l0 = S.passes.empty() ? 0 : S.passes[0].ips_log2;
  int32_t cap = 0;  // the longest first-pass chunk
  if (!S.passes.empty())
    for (int c = 0; c < S.passes[0].n_chunks; c++) cap = std::max(cap, A[S.passes[0].chunk_off + 3 * (size_t)c + 1]);
  line += "P " + std::to_string(P.n_members) + " " + std::to_string(S.passes.size()) + " " + std::to_string(l0) + " " +
          std::to_string(cap) + " " + std::to_string(S.tmp_items);
  return line;
}

std::string run_included(Input& in) {
  const size_t n_jobs = (size_t)in.next();
  std::vector<lsg_job> jobs(n_jobs);
  std::vector<int32_t> status(n_jobs);
  std::vector<size_t> ids(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) {
    jobs[j].sets = nullptr;
    jobs[j].n_sets = (uint32_t)in.next();
    jobs[j].flags = (uint32_t)in.next();
    status[j] = (int32_t)in.next();
    ids[j] = j;
  }
  PkgShape sh;
  const size_t n = shape_jobs(sh, jobs.data(), ids, nullptr);
  std::vector<lsg_job_result> res(n_jobs);
  for (size_t k = 0; k < n_jobs; k++) res[k] = lsg_job_result{status[sh.job_ids[k]], 0};
  const std::vector<uint8_t> mask = included_sets(sh, res.data());
  REQUIRE(mask.size() == n, "one mask byte per staged set");
  std::string line;
  for (size_t k = 0; k < n_jobs; k++) line += std::to_string(sh.jobs[k].first) + " " + std::to_string(sh.jobs[k].count) + " ";
  line += "M ";
  for (uint8_t m : mask) line += m ? "1" : "0";
  return line;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: groupcheck CASES OUT");
  Input in;
  {
    std::ifstream f(argv[1]);
    REQUIRE(f.good(), "cannot read the case file");
    long long x;
    while (f >> x) in.v.push_back(x);
  }
  const size_t n_cases = (size_t)in.next();
  std::ofstream o(argv[2]);
  for (size_t k = 0; k < n_cases; k++) o << (in.next() == 0 ? run_groups(in) : run_included(in)) << "\n";
  REQUIRE(in.at == in.v.size(), "trailing integers in the case file");
  return 0;
}
