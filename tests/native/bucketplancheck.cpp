// bucketplancheck.cpp -- CPU driver of the bucket plan of the signature MSM
// (lodestar_amd/csrc/lsg_plan.hpp plan_buckets, reached through plan_phase as the host does;
// tests/test_msm_buckets_host.py).  No device and no input: every case is built here from a seed.
//
//   bucketplancheck OUT      one text line per case:
//     "<name> sets N groups G new L passes P waves W adds A chain C old L passes P adds A"
//
// Per case the phase is planned twice, with the shipped switches and with msm_fold = false (the
// plan the bucket pass had before: plan_seg's), and both bucket plans are replayed on 64-bit
// integers with + as the operation against sums taken directly from the randomizers' digits.
// The lane-pair additions of a plan are counted here, not taken from the header: chunks in
// launch order, 32 >> ips_log2 to a wave, a wave costing each of its 32 lane pairs its longest
// serial fold (a fold of m members is m - 1 additions) plus one addition per butterfly level.
// Any broken invariant prints a message and exits nonzero.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../lodestar_amd/csrc/lsg_plan.hpp"

using namespace lsgp;

namespace {

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "bucketplancheck: %s\n", m.c_str());
  exit(2);
}
#define REQUIRE(c, m) \
  do {                \
    if (!(c)) die(m); \
  } while (0)

uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct Replay {
  std::vector<uint64_t> sums;
  size_t adds = 0, waves = 0;
  int chain = 0;
};

// the plan as the kernels read it (k_msm_bucket_seg / k_seg_reduce: pass 0 through the index list,
// later passes over the tmp buffer the pass before wrote), with the limits a chunk must keep
Replay replay(const std::vector<int32_t>& A, const SegPlan& P, const std::vector<uint64_t>& x, size_t n_dst, int fold_wide,
              bool sorted_first) {
  Replay R;
  R.sums.assign(n_dst, 0);
  std::vector<uint8_t> wr(n_dst, 0), tw[3];
  std::vector<uint64_t> tmp[3];
  REQUIRE(P.op == 1 && P.has_idx, "the bucket plan is a G2 sum over an index list");
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    REQUIRE(q.ips_log2 >= 0 && q.ips_log2 <= 5, "lane pairs per chunk beyond a wave");
    REQUIRE((k == 0) == (q.src == 0) && (q.tmp_out == 1 || q.tmp_out == 2) && q.src != q.tmp_out, "pass buffers");
    const int32_t cap = (int32_t)(std::max(SEG_FOLD, fold_wide) << q.ips_log2);
    tmp[q.tmp_out].assign(P.tmp_items, 0);
    tw[q.tmp_out].assign(P.tmp_items, 0);
    REQUIRE(q.chunk_off + 3 * (size_t)q.n_chunks <= A.size(), "chunk list outside the arena");
    const size_t per_wave = (size_t)32 >> q.ips_log2;
    int pass_chain = 0;
    int32_t before = 0x7fffffff, longest = 0;
    for (int c = 0; c < q.n_chunks; c++) {
      const int32_t off = A[q.chunk_off + 3 * c], len = A[q.chunk_off + 3 * c + 1], out = A[q.chunk_off + 3 * c + 2];
      REQUIRE(off >= 0 && len >= 0 && len <= cap, "chunk longer than its lane pairs fold");
      if (k == 0 && sorted_first) REQUIRE(len <= before, "first-pass chunks not by descending length");
      before = len;
      uint64_t acc = 0;
      for (int32_t j = 0; j < len; j++) {
        size_t e = (size_t)(off + j);
        if (k == 0) {
          REQUIRE(P.idx_off + e < A.size() && A[P.idx_off + e] >= 0, "idx outside the arena");
          e = (size_t)A[P.idx_off + e];
          REQUIRE(e < x.size(), "element outside the input");
          acc += x[e];
        } else {
          REQUIRE(e < tmp[q.src].size() && tw[q.src][e] == 1, "tmp entry read before it was written");
          acc += tmp[q.src][e];
        }
      }
      if (out >= 0) {
        REQUIRE((size_t)out < n_dst && !wr[out], "result written twice or out of range");
        R.sums[out] = acc;
        wr[out] = 1;
      } else {
        const size_t t = (size_t)(-out - 1);
        REQUIRE(t < P.tmp_items && !tw[q.tmp_out][t], "tmp entry written twice or out of range");
        tmp[q.tmp_out][t] = acc;
        tw[q.tmp_out][t] = 1;
      }
      // the cost of the wave this chunk closes
      longest = std::max(longest, len);
      if (((size_t)c + 1) % per_wave == 0 || c + 1 == q.n_chunks) {
        const int ips = 1 << q.ips_log2;
        const int cost = (longest > 0 ? (longest + ips - 1) / ips - 1 : 0) + q.ips_log2;
        R.adds += (size_t)32 * (size_t)cost;
        pass_chain = std::max(pass_chain, cost);
        longest = 0;
      }
    }
    R.waves = std::max(R.waves, ((size_t)q.n_chunks + per_wave - 1) / per_wave);
    R.chain += pass_chain;
  }
  for (size_t b = 0; b < n_dst; b++) REQUIRE(wr[b], "bucket never summed");
  return R;
}

struct Case {
  const char* name;
  std::vector<size_t> group_len;  // MSM groups, in set order
  int rnd_mode;                   // 0 random, 1 all equal (0x0101..01), 2 random with zero digits
  int want_passes;  // the passes of the new plan (never more than the present plan's)
  int want_ips;  // >= 0: the first pass of both plans must take it
  bool modelled;  // some bucket holds more than SEG_FOLD members: plan_buckets' model plans the pass
};

void run_case(const Case& cs, FILE* out) {
  size_t n = 0;
  PhasePlan Ph[2];
  for (size_t len : cs.group_len) {
    Grp g;
    g.first = n;
    g.len = len;
    g.msm = true;
    for (PhasePlan& p : Ph) p.groups.push_back(g);
    n += len;
  }
  uint64_t sd = 0xB0C4E7 + 131 * (uint64_t)n + (uint64_t)cs.rnd_mode;
  std::vector<uint64_t> rnd(n), x(n);
  for (size_t i = 0; i < n; i++) {
    uint64_t r = splitmix64(sd);
    if (cs.rnd_mode == 1) r = 0x0101010101010101ull;
    if (cs.rnd_mode == 2) {  // about a third of the 4-bit digits are zero
      const uint64_t m = splitmix64(sd) & splitmix64(sd);
      for (int d = 0; d < 16; d++)
        if (((m >> (4 * d)) & 3u) == 0) r &= ~(0xfull << (4 * d));
    }
    if (r == 0) r = 1;
    rnd[i] = r;
    x[i] = splitmix64(sd);
  }
  // the buckets, directly: group g's window w of c bits, digit d != 0, numbered as plan_phase does
  std::vector<uint64_t> want;
  for (size_t g = 0; g < cs.group_len.size(); g++) {
    const int c = msm_window_bits(cs.group_len[g]), nw = 64 / c;
    const size_t base = want.size(), nd = ((size_t)1 << c) - 1;
    want.resize(base + (size_t)nw * nd, 0);
    for (size_t i = Ph[0].groups[g].first; i < Ph[0].groups[g].first + cs.group_len[g]; i++)
      for (int w = 0; w < nw; w++) {
        const uint64_t d = (rnd[i] >> (c * w)) & (uint64_t)nd;
        if (d) want[base + (size_t)w * nd + d - 1] += x[i];
      }
  }
  Replay R[2];
  std::vector<int32_t> arena[2];
  for (int v = 0; v < 2; v++) {
    Switches sw;
    sw.msm_fold = v == 0;
    std::vector<int32_t> A(5, -1);  // (the arena is not empty before the plan)
    plan_phase(A, rnd, 4, sw, Ph[v]);
    REQUIRE(Ph[v].n_msm == cs.group_len.size(), "MSM groups");
    // with a bucket of more than SEG_FOLD members the shipped plan is the model's, its first pass in
    // descending order; else it is plan_seg's own plan, word for word (checked below)
    R[v] = replay(A, Ph[v].buckets, x, want.size(), sw.seg_fold_wide, v == 0 && cs.modelled);
    arena[v] = A;
    REQUIRE(R[v].sums == want, std::string(cs.name) + ": bucket sums differ from the direct sums");
    // the bit sums read the buckets by number: the same lists whatever the bucket plan
    REQUIRE(!Ph[v].bits.passes.empty(), "no bit sums");
  }
  const SegPlan &N = Ph[0].buckets, &O = Ph[1].buckets;
  // the header's length-only model prices both plans as the replay counts them, and its choice is the plan's
  std::vector<int32_t> lens(want.size(), 0);
  for (size_t g = 0, base = 0; g < cs.group_len.size(); g++) {
    const int c = msm_window_bits(cs.group_len[g]), nw = 64 / c;
    const size_t nd = ((size_t)1 << c) - 1;
    for (size_t i = Ph[0].groups[g].first; i < Ph[0].groups[g].first + cs.group_len[g]; i++)
      for (int w = 0; w < nw; w++) {
        const uint64_t d = (rnd[i] >> (c * w)) & (uint64_t)nd;
        if (d) lens[base + (size_t)w * nd + d - 1]++;
      }
    base += (size_t)nw * nd;
  }
  int32_t longest = 0;
  for (int32_t l : lens) longest = std::max(longest, l);
  REQUIRE((longest > SEG_FOLD) == cs.modelled, std::string(cs.name) + ": the case is on the other side of the model's threshold");
  if (!cs.modelled) {
    REQUIRE(arena[0] == arena[1], std::string(cs.name) + ": a small group's plan is not plan_seg's");
    fprintf(out, "%s sets %zu groups %zu new %d passes %zu waves %zu adds %zu chain %d old %d passes %zu adds %zu\n", cs.name, n,
            cs.group_len.size(), N.passes[0].ips_log2, N.passes.size(), R[0].waves, R[0].adds, R[0].chain, O.passes[0].ips_log2,
            O.passes.size(), R[1].adds);
    REQUIRE((int)N.passes.size() == cs.want_passes && N.passes[0].ips_log2 == cs.want_ips, std::string(cs.name) + ": small group moved");
    return;
  }
  const SegCost mo = bucket_cost(lens, -1, SEG_FOLD_WIDE);
  REQUIRE(mo.adds == R[1].adds && mo.chain == R[1].chain && mo.passes == (int)O.passes.size(), std::string(cs.name) + ": model of the present plan");
  REQUIRE(bucket_ips(lens, SEG_FOLD_WIDE) == N.passes[0].ips_log2, std::string(cs.name) + ": the plan does not take the model's choice");
  std::sort(lens.begin(), lens.end(), std::greater<int32_t>());
  const SegCost mn = bucket_cost(lens, N.passes[0].ips_log2, SEG_FOLD_WIDE);
  REQUIRE(mn.adds == R[0].adds && mn.chain == R[0].chain && mn.waves == R[0].waves && mn.passes == (int)N.passes.size(),
          std::string(cs.name) + ": model of the new plan");
  if (cs.want_ips < 0) REQUIRE(R[0].adds < R[1].adds, std::string(cs.name) + ": the new plan saves nothing");
  REQUIRE((int)N.passes.size() == cs.want_passes && N.passes.size() <= O.passes.size(), std::string(cs.name) + ": passes");
  if (cs.want_ips >= 0)
    REQUIRE(N.passes[0].ips_log2 == cs.want_ips && O.passes[0].ips_log2 == cs.want_ips,
            std::string(cs.name) + ": lane pairs per bucket moved");
  fprintf(out, "%s sets %zu groups %zu new %d passes %zu waves %zu adds %zu chain %d old %d passes %zu adds %zu\n", cs.name, n,
          cs.group_len.size(), N.passes[0].ips_log2, N.passes.size(), R[0].waves, R[0].adds, R[0].chain, O.passes[0].ips_log2,
          O.passes.size(), R[1].adds);
  if (n == 32768 && cs.rnd_mode == 0)
    REQUIRE((double)R[0].adds <= 0.65 * (double)R[1].adds, "32,768 sets: modelled additions above 0.65 of the present plan's");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: bucketplancheck OUT");
  FILE* out = fopen(argv[1], "w");
  if (!out) die("cannot open the output");
  const Case cases[] = {
      {"random256", {256}, 0, 1, 0, false},
      {"random257", {257}, 0, 1, 0, false},
      {"random4096", {4096}, 0, 1, -1, true},
      {"random32768", {32768}, 0, 1, -1, true},
      {"equal4096", {4096}, 1, 2, -1, true},
      {"zerodigits4096", {4096}, 2, 1, -1, true},
      {"widths2048+255", {2048, 255}, 0, 1, -1, true},
  };
  for (const Case& c : cases) run_case(c, out);
  if (fclose(out) != 0) die("write failed");
  printf("%zu\n", sizeof(cases) / sizeof(cases[0]));
  return 0;
}
