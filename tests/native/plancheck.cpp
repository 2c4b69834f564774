// plancheck.cpp -- CPU driver of lodestar_amd/csrc/lsg_plan.hpp (tests/test_plan_host.py).
// No device: the per-set status a package would read back is given as integers, the group
// checks are a fake (a group passes iff each of its sets without an error is valid), and the
// planned reductions are executed on 64-bit integers with + as the operation.
//
//   plancheck CASES OUT     CASES: whitespace-separated integers, OUT: one text line per case
//
// CASES = n_cases, then per case
//   1 K msm_min package_group sub_groups nb_merge b0_min b0_run lone_ok seed n_jobs n_bounds
//     bounds[n_bounds]                 (sub-package job bounds of a coalesced launch, or none)
//     per job: flags n_sets, per set: valid sig_err pk_inf n_keys key_err[n_keys]
//     -> "J status code ..  S retries success key_error key_error_job  U (the same per
//        sub-package) ..  C check_calls"
//   2 op fold_wide has_idx n_specs (len count)[n_specs]      segments for plan_seg
//     -> "seg ok passes P"
//   3 K msm_min package_group sub_groups nb_merge b0_min b0_run lone_ok rnd_mode seed ...
//     case 1 with chosen randomizers for the scaled sets (case 1 is rnd_mode 0: splitmix64 | 1):
//     1 all 0x0101010101010101 (eight buckets hold every set), 2 all 2^63 (one bit sum is not
//     empty), 3 all 2^64 - 1, 4 (1 + i mod 255) << 24 (every bucket of one window, no other)
//     -> the line of case 1 followed by " P passes" (of phase A's bucket plan; 0: no MSM group)
// Any broken invariant prints a message and exits nonzero.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <string>

#include "../../lodestar_amd/csrc/lsg_plan.hpp"

using namespace lsgp;

namespace {

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "plancheck: %s\n", m.c_str());
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

struct Input {
  std::vector<long long> v;
  size_t at = 0;
  long long next() {
    REQUIRE(at < v.size(), "case file ends early");
    return v[at++];
  }
};

// One planned reduction as lsgk::seg_reduce reads it: per pass n_chunks triples (off, len,
// dst) at chunk_off; pass 0 reads src (through the idx list when the plan has one), later
// passes a tmp buffer; dst >= 0 goes to the result, dst < 0 to tmp[-dst - 1] of tmp_out.
// Returns the results by dst index; every result and every tmp entry is written exactly once
// and nothing is read before it is written.
std::vector<uint64_t> run_seg(const std::vector<int32_t>& A, const SegPlan& P, const std::vector<uint64_t>& src,
                              size_t n_dst, int fold_wide, std::vector<uint8_t>* written) {
  std::vector<uint64_t> dst(n_dst, 0), tmp[3];
  std::vector<uint8_t> wr(n_dst, 0), tw[3];
  for (size_t k = 0; k < P.passes.size(); k++) {
    const SegPass& q = P.passes[k];
    REQUIRE(q.ips_log2 >= 0 && q.ips_log2 <= 5, "lane pairs per chunk beyond a wave");
    REQUIRE((k == 0) == (q.src == 0) && (q.tmp_out == 1 || q.tmp_out == 2) && q.src != q.tmp_out, "pass buffers");
    const int fold = P.op == 2 ? SEG_FOLD_FP12 : std::max(SEG_FOLD, fold_wide);  // (the most a pass may fold)
    tmp[q.tmp_out].assign(P.tmp_items, 0);
    tw[q.tmp_out].assign(P.tmp_items, 0);
    REQUIRE(q.chunk_off + 3 * (size_t)q.n_chunks <= A.size(), "chunk list outside the arena");
    for (int c = 0; c < q.n_chunks; c++) {
      const int32_t off = A[q.chunk_off + 3 * c], len = A[q.chunk_off + 3 * c + 1], out = A[q.chunk_off + 3 * c + 2];
      REQUIRE(off >= 0 && len >= 0 && len <= (fold << q.ips_log2), "chunk longer than its lane pairs fold");
      uint64_t acc = 0;
      for (int32_t j = 0; j < len; j++) {
        size_t e = (size_t)(off + j);
        if (k == 0) {
          if (P.has_idx) {
            REQUIRE(P.idx_off + e < A.size() && A[P.idx_off + e] >= 0, "idx outside the arena");
            e = (size_t)A[P.idx_off + e];
          }
          REQUIRE(e < src.size(), "element outside the input");
          acc += src[e];
        } else {
          REQUIRE(e < tmp[q.src].size() && tw[q.src][e] == 1, "tmp entry read before it was written");
          acc += tmp[q.src][e];
        }
      }
      if (out >= 0) {
        REQUIRE((size_t)out < n_dst && !wr[out], "result written twice or out of range");
        dst[out] = acc;
        wr[out] = 1;
      } else {
        const size_t t = (size_t)(-out - 1);
        REQUIRE(t < P.tmp_items && !tw[q.tmp_out][t], "tmp entry written twice or out of range");
        tmp[q.tmp_out][t] = acc;
        tw[q.tmp_out][t] = 1;
      }
    }
  }
  if (written) *written = wr;
  return dst;
}

// ---- case 2: plan_seg against the direct sums
void seg_case(Input& in, FILE* out) {
  const int op = (int)in.next(), fold_wide = (int)in.next();
  const bool has_idx = in.next() != 0;
  std::vector<int32_t> off, len;
  int32_t tot = 0;
  for (long long k = in.next(); k > 0; k--) {
    const int32_t l = (int32_t)in.next();
    for (long long c = in.next(); c > 0; c--) {
      off.push_back(tot);
      len.push_back(l);
      tot += l;
    }
  }
  uint64_t sd = 0x5EED + (uint64_t)tot;
  std::vector<uint64_t> src((size_t)tot + 3);
  for (auto& x : src) x = splitmix64(sd);
  std::vector<int32_t> A(7, -1);  // (the arena is not empty before the plan)
  const size_t idx_off = A.size();
  std::vector<size_t> elem((size_t)tot);  // segment element e is input element elem[e]
  for (size_t e = 0; e < elem.size(); e++) elem[e] = has_idx ? (e * 7919 + 1) % src.size() : e;
  if (has_idx)
    for (size_t e : elem) A.push_back((int32_t)e);
  const int32_t dst_base = 3;
  const SegPlan P = plan_seg(A, op, off, len, has_idx, idx_off, dst_base, fold_wide);
  std::vector<uint8_t> wr;
  const std::vector<uint64_t> got = run_seg(A, P, src, (size_t)dst_base + len.size(), fold_wide, &wr);
  for (size_t s = 0; s < len.size(); s++) {
    uint64_t want = 0;
    for (int32_t j = 0; j < len[s]; j++) want += src[elem[(size_t)(off[s] + j)]];
    REQUIRE(wr[(size_t)dst_base + s], "segment never reduced");
    REQUIRE(got[(size_t)dst_base + s] == want, "segment sum differs from the direct sum");
  }
  for (int32_t d = 0; d < dst_base; d++) REQUIRE(!wr[(size_t)d], "result below dst_base written");
  fprintf(out, "seg ok passes %zu\n", P.passes.size());
}

// ---- the invariants of one planned phase (plan_phase), on integers
void check_phase(const std::vector<int32_t>& A, const PhasePlan& Ph, const std::vector<uint64_t>& rnd, size_t n_sets,
                 const PhasePlan* phA, int fold_wide) {
  const size_t ng = Ph.groups.size();
  uint64_t sd = 77 + ng;
  // items: each lies in one sub-range (or group), and a group's items cover its sets once
  const std::vector<int32_t>& itf = Ph.reuse_items ? phA->it_first : Ph.it_first;
  const std::vector<int32_t>& itc = Ph.reuse_items ? phA->it_cnt : Ph.it_cnt;
  std::vector<ItemRange> gi(ng);
  if (Ph.reuse_items) {
    gi = Ph.given;
  } else {
    size_t it = 0;
    for (size_t g = 0; g < ng; g++) {
      std::vector<Range> rs;
      if (g < Ph.sub.size() && !Ph.sub[g].empty())
        rs = Ph.sub[g];
      else
        rs.push_back({Ph.groups[g].first, Ph.groups[g].first + Ph.groups[g].len});
      gi[g].first = (int32_t)it;
      for (const Range& r : rs)
        for (size_t at = r.first; at < r.second;) {
          REQUIRE(it < itf.size() && (size_t)itf[it] == at && itc[it] >= 1, "items do not follow the sub-ranges");
          at += (size_t)itc[it++];
          REQUIRE(at <= r.second, "an item crosses a group or a sub-range");
        }
      gi[g].second = (int32_t)it;
    }
    REQUIRE(it == itf.size() && it == Ph.n_items && Ph.term_base == Ph.n_items, "item count");
  }
  for (size_t g = 0; g < ng; g++) {  // (given items too: exactly the group's sets, in order)
    size_t at = Ph.groups[g].first;
    for (int32_t it = gi[g].first; it < gi[g].second; it++) {
      REQUIRE(it >= 0 && (size_t)it < itf.size() && (size_t)itf[(size_t)it] == at, "a group's items do not cover its sets");
      at += (size_t)itc[(size_t)it];
    }
    REQUIRE(at == Ph.groups[g].first + Ph.groups[g].len, "a group's items do not cover its sets");
  }
  // products: every item of the group once plus its own term slot
  std::vector<uint64_t> fall(Ph.term_base + ng);
  for (auto& x : fall) x = splitmix64(sd);
  const std::vector<uint64_t> F = run_seg(A, Ph.prod, fall, ng, fold_wide, nullptr);
  for (size_t g = 0; g < ng; g++) {
    uint64_t want = fall[Ph.term_base + g];
    for (int32_t it = gi[g].first; it < gi[g].second; it++) want += fall[(size_t)it];
    REQUIRE(F[g] == want, "a group's product list");
  }
  // signature sums: bucket MSM groups first (sum r_i x_i through buckets, bit sums and Horner
  // with weights 2^k), then the contiguous sums
  std::vector<uint64_t> x(n_sets);
  for (auto& v : x) v = splitmix64(sd);
  REQUIRE(Ph.n_msm <= ng, "msm count");
  for (size_t g = 0; g < ng; g++) REQUIRE(Ph.groups[g].msm == (g < Ph.n_msm), "MSM groups must come first");
  if (Ph.n_msm) {
    size_t nb = 0;
    for (size_t g = 0; g < Ph.n_msm; g++) {
      const int c = msm_window_bits(Ph.groups[g].len);
      nb += (size_t)(64 / c) * ((1u << c) - 1);
    }
    const std::vector<uint64_t> bkt = run_seg(A, Ph.buckets, x, nb, fold_wide, nullptr);
    const std::vector<uint64_t> bits = run_seg(A, Ph.bits, bkt, 64 * Ph.n_msm, fold_wide, nullptr);
    for (size_t g = 0; g < Ph.n_msm; g++) {
      uint64_t got = 0, want = 0;
      for (int k = 0; k < 64; k++) got += bits[64 * g + (size_t)k] << k;
      for (size_t i = Ph.groups[g].first; i < Ph.groups[g].first + Ph.groups[g].len; i++) want += rnd[i] * x[i];
      REQUIRE(got == want, "bucket MSM does not reproduce sum r_i x_i");
    }
  }
  if (Ph.n_msm < ng) {
    const std::vector<uint64_t> S = run_seg(A, Ph.sums, x, ng, fold_wide, nullptr);
    for (size_t g = Ph.n_msm; g < ng; g++) {
      uint64_t want = 0;
      for (size_t i = Ph.groups[g].first; i < Ph.groups[g].first + Ph.groups[g].len; i++) want += x[i];
      REQUIRE(S[g] == want, "a scaled group's sum");
    }
  }
}

// the randomizer of scaled set i under rnd_mode (the header lists the modes)
uint64_t chosen_rnd(int mode, size_t i, uint64_t& sd) {
  switch (mode) {
    case 0: return splitmix64(sd) | 1;
    case 1: return 0x0101010101010101ull;
    case 2: return 1ull << 63;
    case 3: return ~0ull;
    case 4: return (uint64_t)(1 + i % 255) << 24;
  }
  die("unknown rnd_mode");
}

// ---- cases 1 and 3: one package through plan_groups, plan_phase and resolve_package
void verdict_case(Input& in, FILE* out, bool with_mode) {
  const int K = (int)in.next();
  Switches sw;
  sw.msm_min_group = (size_t)in.next();
  sw.package_group = in.next() != 0;
  sw.sub_groups = in.next() != 0;
  sw.nb_merge = in.next() != 0;
  sw.b0_min = (size_t)in.next();
  sw.b0_run = (size_t)in.next();
  const bool lone_ok = in.next() != 0;
  const int rnd_mode = with_mode ? (int)in.next() : 0;
  uint64_t sd = (uint64_t)in.next();
  const size_t nj = (size_t)in.next();
  std::vector<size_t> subs((size_t)in.next());
  for (auto& b : subs) b = (size_t)in.next();
  // the package as the caller gives it (caller order), then in staging order
  struct SetIn {
    bool valid;
    int32_t sig_err, pinf;
    std::vector<int32_t> key_err;
  };
  std::vector<lsg_job> jobs(nj);
  std::vector<std::vector<SetIn>> sets(nj);
  std::vector<size_t> ids(nj);
  for (size_t j = 0; j < nj; j++) {
    ids[j] = j;
    jobs[j].sets = nullptr;
    jobs[j].flags = (uint32_t)in.next();
    jobs[j].n_sets = (uint32_t)in.next();
    sets[j].resize(jobs[j].n_sets);
    for (SetIn& q : sets[j]) {
      q.valid = in.next() != 0;
      q.sig_err = (int32_t)in.next();
      q.pinf = (int32_t)in.next();
      q.key_err.resize((size_t)in.next());
      for (auto& e : q.key_err) e = (int32_t)in.next();
    }
  }
  PkgShape sh;
  const size_t n = shape_jobs(sh, jobs.data(), ids, subs.empty() ? nullptr : &subs);
  // what the device reads back: a validated key that fails is its set's error (it beats the
  // signature's, the first bad key in order gives it); a set without keys has pinf 2
  std::vector<int32_t> err(n, 0), pkerr;
  std::vector<uint8_t> valid(n, 0);
  SetStatus ss;
  ss.pinf.assign(n, 0);
  sh.pk_cnt.assign(n, 0);
  sh.pk_first.assign(n, 0);
  bool any_kv = false;
  for (size_t j = 0; j < nj; j++) any_kv = any_kv || (jobs[j].flags & LSG_JOB_VALIDATE_KEYS) != 0;
  if (any_kv) sh.kv_set.assign(n, 0);
  for (int pass = 0; pass < 2; pass++)  // keys are staged in set order
    for (size_t j = 0; j < nj; j++) {
      if (batchable(sh.jobs[j]) != (pass == 0)) continue;
      for (size_t q = 0; q < sets[j].size(); q++) {
        const SetIn& S = sets[j][q];
        const size_t i = sh.jobs[j].first + q;
        valid[i] = S.valid;
        err[i] = S.sig_err;
        ss.pinf[i] = S.key_err.empty() ? 2 : (uint8_t)(S.pinf != 0);
        sh.pk_cnt[i] = (uint32_t)S.key_err.size();
        sh.pk_first[i] = (uint32_t)pkerr.size();
        pkerr.insert(pkerr.end(), S.key_err.begin(), S.key_err.end());
        if ((jobs[j].flags & LSG_JOB_VALIDATE_KEYS) && !S.key_err.empty()) {
          sh.kv_set[i] = 1;
          for (size_t k = S.key_err.size(); k-- > 0;)
            if (S.key_err[k]) err[i] = S.key_err[k];
        }
      }
    }
  bool kv = false;
  for (uint8_t b : sh.kv_set) kv = kv || b;
  if (!kv) sh.kv_set.clear();
  pkerr.push_back(0);
  ss.err = err.data();
  ss.pkerr = pkerr.data();

  GroupPlan gp = plan_groups(sh, sw, lone_ok);
  REQUIRE(gp.noscale.size() == n, "noscale size");
  std::vector<uint64_t> rnd(n);
  for (size_t i = 0; i < n; i++) rnd[i] = gp.noscale[i] ? 0 : chosen_rnd(rnd_mode, i, sd);
  // phase-A groups: disjoint, MSM groups first, every set with a job in exactly one group;
  // an unscaled set is alone in its group
  std::vector<int> set_group(n, -1);
  for (size_t g = 0; g < gp.groups.size(); g++)
    for (size_t i = gp.groups[g].first; i < gp.groups[g].first + gp.groups[g].len; i++) {
      REQUIRE(i < n && set_group[i] < 0, "phase-A groups overlap");
      set_group[i] = (int)g;
      REQUIRE(!gp.noscale[i] || gp.groups[g].len == 1, "an unscaled set shares its group");
    }
  for (size_t i = 0; i < n; i++) REQUIRE(set_group[i] >= 0, "a set is in no phase-A group");
  PhasePlan A;
  A.groups = gp.groups;
  A.sub = gp.sub;
  std::vector<int32_t> arena;
  plan_phase(arena, rnd, K, sw, A);
  group_items(gp, sh, A);
  check_phase(arena, A, rnd, n, nullptr, sw.seg_fold_wide);

  auto passes = [&](const Grp& g) {
    for (size_t i = g.first; i < g.first + g.len; i++)
      if (set_error(ss, i) == 0 && !valid[i]) return false;
    return true;
  };
  std::vector<int32_t> vA;
  for (const Grp& g : A.groups) vA.push_back(passes(g));
  size_t calls = 0;
  const CheckFn check = [&](const std::vector<Grp>& groups, const std::vector<ItemRange>* given, std::vector<int32_t>& v) {
    v.assign(groups.size(), 0);
    if (groups.empty()) return LSG_OK;
    calls++;
    // the phase as lsg_host.hip plans it: MSM groups (sets of phase-A MSM groups only) first
    PhasePlan Ph;
    std::vector<size_t> order;
    for (int m = 1; m >= 0; m--)
      for (size_t g = 0; g < groups.size(); g++) {
        bool msm = groups[g].len >= std::max(sw.msm_min_group, (size_t)2);
        for (size_t i = groups[g].first; msm && i < groups[g].first + groups[g].len; i++) msm = A.groups[(size_t)set_group[i]].msm;
        if (msm != (m == 1)) continue;
        order.push_back(g);
        Ph.groups.push_back(groups[g]);
        Ph.groups.back().msm = msm;
        if (given) Ph.given.push_back((*given)[g]);
      }
    size_t singles = 0;
    for (const Grp& g : groups) singles += g.len == 1 ? 1 : 0;
    if (given) {
      Ph.reuse_items = true;
      Ph.n_items = A.n_items;
      Ph.term_base = A.n_items + A.groups.size();
    }
    std::vector<int32_t> arena2;
    plan_phase(arena2, rnd, !given && 2 * singles >= groups.size() ? 1 : K, sw, Ph);
    check_phase(arena2, Ph, rnd, n, &A, sw.seg_fold_wide);  // (with given: the items cover exactly the group's sets)
    for (size_t g = 0; g < groups.size(); g++) {
      REQUIRE(groups[g].len > 0 && groups[g].first + groups[g].len <= n, "a checked group is empty or out of range");
      v[g] = passes(groups[g]);
    }
    return LSG_OK;
  };
  size_t key_job = 0;
  const int32_t pkfail = sh.n_sub ? 0 : first_key_error(sh, ss.pkerr, 0, nj, &key_job);
  std::vector<lsg_job_result> results(nj, lsg_job_result{LSG_INVALID, 0});
  lsg_stats z = lsg_stats(), stats = z;
  std::vector<lsg_stats> sub_stats((size_t)sh.n_sub, z);
  std::vector<int32_t> sub_pkfail((size_t)sh.n_sub, 0);
  const int rc = resolve_package(sh, gp, ss, vA, pkfail, A, sw, check, PkgVerdicts{results, stats, sub_stats, sub_pkfail});
  REQUIRE(rc == LSG_OK, "resolve_package failed");
  for (size_t j = 0; j < nj; j++) fprintf(out, "J %d %d ", results[j].status, results[j].err_code);
  fprintf(out, "S %u %u %d %zu ", stats.batch_retries, stats.batch_sigs_success, pkfail, pkfail ? sh.job_ids[key_job] : 0);
  for (size_t k = 0; k < sub_stats.size(); k++) {
    REQUIRE(sub_pkfail[k] == sub_stats[k].key_error, "sub-package key error");
    fprintf(out, "U %u %u %d %u ", sub_stats[k].batch_retries, sub_stats[k].batch_sigs_success, sub_stats[k].key_error,
            sub_stats[k].key_error_job);
  }
  fprintf(out, "C %zu", calls);
  if (with_mode) fprintf(out, " P %zu", A.n_msm ? A.buckets.passes.size() : (size_t)0);
  fprintf(out, "\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: plancheck CASES OUT");
  Input in;
  {
    std::ifstream f(argv[1]);
    REQUIRE(f.good(), "cannot read the case file");
    for (long long x; f >> x;) in.v.push_back(x);
  }
  FILE* out = fopen(argv[2], "w");
  REQUIRE(out != nullptr, "cannot write the output file");
  for (long long k = in.next(); k > 0; k--) {
    const long long kind = in.next();
    if (kind == 1 || kind == 3)
      verdict_case(in, out, kind == 3);
    else if (kind == 2)
      seg_case(in, out);
    else
      die("unknown case kind");
  }
  REQUIRE(in.at == in.v.size(), "trailing integers in the case file");
  fclose(out);
  return 0;
}
