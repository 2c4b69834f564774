// committeemulticheck.cpp -- CPU driver of the multi-committee set policy (LSG_PK_BITS_MULTI) in
// lodestar_amd/csrc/lsg_plan.hpp and of the walk across parts in lsg_bits.h
// (tests/test_committee_multi_plan_host.py).  No device: committee members are small integers
// standing in for keys, "addition" is addition mod the prime 2^61 - 1, the identity is 0.  Each
// case's sets are staged (multi_stage_set: the shifted copy of every part), planned
// (plan_multi) and then executed as k_pk_agg_bits_multi executes them: per lane pair the walk
// across the set's parts with the carried skip, members of complement parts negated, the
// complement parts' stored sums dealt round robin, the butterfly within the wave.
//
//   committeemulticheck CASES OUT   CASES: whitespace-separated integers, OUT: one line per case
//
// CASES = n_cases, then per case
//   n_committees, per committee: len member[len]
//   n_sets, per set: k id[k]  n_bits  n_bytes byte[n_bytes]     (n_bytes >= ceil(n_bits / 8))
// OUT per case: per set "result pairs first_pair items complement_parts", then "P n_pairs fold".
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
  fprintf(stderr, "committeemulticheck: %s\n", m.c_str());
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
uint64_t neg(uint64_t a) { return (PRIME - a % PRIME) % PRIME; }
bool bit(const std::vector<uint8_t>& f, uint64_t k) { return (f[k >> 3] >> (k & 7)) & 1; }

std::string run_case(Input& in) {
  const size_t n_cm = (size_t)in.next();
  std::vector<uint32_t> cm_off(n_cm), cm_len(n_cm);
  std::vector<uint64_t> cm_rows, cm_sum(n_cm, 0);
  for (size_t c = 0; c < n_cm; c++) {
    cm_len[c] = (uint32_t)in.next();
    cm_off[c] = (uint32_t)cm_rows.size();
    for (uint32_t k = 0; k < cm_len[c]; k++) {
      const uint64_t m = (uint64_t)in.next();
      cm_rows.push_back(m);
      cm_sum[c] = add(cm_sum[c], m);
    }
  }
  const size_t n_sets = (size_t)in.next();
  std::vector<std::vector<uint32_t>> ids(n_sets), lens(n_sets);
  // the caller's field in a buffer of exactly its bytes: a read past it is a sanitizer report
  std::vector<std::vector<uint8_t>> fields(n_sets);
  std::vector<uint32_t> n_bits(n_sets);
  size_t words = 0;
  for (size_t i = 0; i < n_sets; i++) {
    const size_t k = (size_t)in.next();
    REQUIRE(k <= LSG_MAX_SET_COMMITTEES, "more committees than a set may list");
    uint64_t total = 0;
    for (size_t e = 0; e < k; e++) {
      ids[i].push_back((uint32_t)in.next());
      REQUIRE(ids[i].back() < n_cm, "unknown committee");
      lens[i].push_back(cm_len[ids[i].back()]);
      total += lens[i].back();
    }
    n_bits[i] = (uint32_t)in.next();
    REQUIRE(n_bits[i] == total, "a set's bit count is the sum of its committees' lengths");
    const size_t nb = (size_t)in.next();
    REQUIRE(nb >= ((size_t)n_bits[i] + 7) / 8, "bitfield shorter than n_bits");
    fields[i].resize(nb);
    for (size_t q = 0; q < nb; q++) fields[i][q] = (uint8_t)in.next();
    // the words its staged parts take: a part without a participant is left out, a set
    // without one stages nothing
    uint64_t off = 0;
    for (size_t e = 0; e < k; off += lens[i][e], e++) {
      uint32_t p = 0;
      for (uint32_t q = 0; q < lens[i][e]; q++) p += bit(fields[i], off + q);
      REQUIRE(bits_count_range(fields[i].data(), off, lens[i][e]) == p, "bits_count_range differs from the bits");
      if (p) words += bits_words(lens[i][e]);
    }
  }
  // staging, exactly sized: a write past a part's words is an AddressSanitizer report
  std::vector<uint32_t> arena(words, 0xdeadbeefu);
  std::vector<MultiSet> sets;
  std::vector<MultiPart> parts;
  size_t bw = 0;
  for (size_t i = 0; i < n_sets; i++) {
    sets.push_back(multi_stage_set(ids[i].data(), lens[i].data(), (uint32_t)ids[i].size(), fields[i].data(), n_bits[i],
                                   (int32_t)i, arena.data(), &bw, parts));
    // every staged part is the shifted copy of its run, the tail of its last word zero
    const MultiSet& m = sets.back();
    uint64_t off = 0;
    size_t at = m.first_part;
    uint32_t p_total = 0;
    for (size_t e = 0; e < ids[i].size(); off += lens[i][e], e++) {
      uint32_t p = 0;
      for (uint32_t q = 0; q < lens[i][e]; q++) p += bit(fields[i], off + q);
      p_total += p;
      if (!p) continue;
      REQUIRE(at < m.first_part + m.n_parts, "a part with participants was not staged");
      const MultiPart& Q = parts[at++];
      REQUIRE(Q.committee == ids[i][e] && Q.n_bits == lens[i][e] && Q.p == p, "part record differs from its committee");
      for (size_t w = 0; w < bits_words(Q.n_bits); w++) {
        uint32_t want = 0;
        for (uint32_t b = 0; b < 32 && 32 * w + b < Q.n_bits; b++) want |= (uint32_t)bit(fields[i], off + 32 * w + b) << b;
        REQUIRE(arena[Q.word_off + w] == want, "shifted copy differs from the caller's bits");
      }
    }
    REQUIRE(at == m.first_part + m.n_parts && m.p == p_total, "staged parts differ from the parts with participants");
  }
  REQUIRE(bw == words, "arena words in use differ from the staged parts'");
  std::vector<int32_t> A;
  A.push_back(12345);  // (the plan does not start at word 0 of its arena)
  const MultiPlan P = plan_multi(A, sets, parts);
  REQUIRE(P.n_sets == n_sets, "one plan entry per set");
  const int32_t* set_plan = A.data() + P.set_off;
  const int32_t* part_plan = A.data() + P.part_off;
  const int32_t* pair_set = A.data() + P.pair_off;
  REQUIRE(P.part_off == P.set_off + MULTI_SET_WORDS * n_sets && P.pair_off == P.part_off + MULTI_PART_WORDS * parts.size(),
          "plan ranges are not back to back");
  REQUIRE(A.size() == P.pair_off + P.n_pairs, "pair table ends the plan");
  // the launch: waves of 32 lane pairs; pairs past n_pairs are idle
  std::vector<uint64_t> out(n_sets, ~0ull);
  std::vector<uint8_t> written(n_sets, 0);
  std::vector<uint32_t> taken(n_sets, 0);
  for (size_t w0 = 0; w0 < P.n_pairs; w0 += 32) {
    uint64_t acc[32];
    int ips[32], j[32], e[32];
    for (int l = 0; l < 32; l++) {
      acc[l] = 0;
      ips[l] = 1;
      j[l] = 0;
      e[l] = -1;
      const size_t item = w0 + (size_t)l;
      if (item >= P.n_pairs) continue;
      e[l] = pair_set[item];
      REQUIRE(e[l] >= 0 && (size_t)e[l] < n_sets, "pair table entry out of range");
      const int32_t* q = set_plan + MULTI_SET_WORDS * (size_t)e[l];
      REQUIRE((size_t)q[0] + (size_t)q[1] <= parts.size(), "parts outside the part table");
      const int32_t* pp = part_plan + MULTI_PART_WORDS * (size_t)q[0];
      const uint32_t n_parts = (uint32_t)q[1];
      REQUIRE(q[3] >= 0 && q[3] <= 5, "more pairs than a wave holds");
      ips[l] = 1 << q[3];
      j[l] = (int)item - q[4];
      REQUIRE(j[l] >= 0 && j[l] < ips[l], "pair outside its set's range");
      for (uint32_t c = 0; c < n_parts; c++)
        REQUIRE(pp[4 * c + 2] >= 1 && (size_t)pp[4 * c + 1] + bits_words((uint32_t)pp[4 * c + 2]) <= arena.size(),
                "field outside the arena");
      lsg_multi_walk wk = lsg_multi_begin((uint32_t)j[l]);
      for (int32_t m = lsg_multi_next(pp, n_parts, arena.data(), (uint32_t)ips[l], wk); m >= 0;
           m = lsg_multi_next(pp, n_parts, arena.data(), (uint32_t)ips[l], wk)) {
        REQUIRE(wk.c < n_parts, "walk left the set's parts");
        const int32_t* p = pp + MULTI_PART_WORDS * wk.c;
        REQUIRE((uint32_t)m < (uint32_t)p[2], "walk left the field");
        const uint64_t key = cm_rows[cm_off[(uint32_t)p[0]] + (uint32_t)m];
        acc[l] = add(acc[l], (p[3] & 1) ? neg(key) : key);
        taken[(size_t)q[2]]++;
      }
      uint32_t r = 0;
      for (uint32_t c = 0; c < n_parts; c++) {
        const int32_t* p = pp + MULTI_PART_WORDS * c;
        if (!(p[3] & 1)) continue;
        if ((int)(r & (uint32_t)(ips[l] - 1)) == j[l]) {
          acc[l] = add(acc[l], cm_sum[(uint32_t)p[0]]);
          taken[(size_t)q[2]]++;
        }
        r++;
      }
    }
    for (int o = 16; o >= 1; o >>= 1) {
      uint64_t t[32];
      for (int l = 0; l < 32; l++) t[l] = acc[l ^ o];
      for (int l = 0; l < 32; l++)
        if (o < ips[l]) {
          REQUIRE(e[l ^ o] == e[l], "butterfly partner belongs to another set");
          acc[l] = add(acc[l], t[l]);
        }
    }
    for (int l = 0; l < 32; l++) {
      if (e[l] < 0 || j[l] != 0) continue;
      const int32_t* q = set_plan + MULTI_SET_WORDS * (size_t)e[l];
      REQUIRE(q[2] >= 0 && (size_t)q[2] < n_sets && !written[(size_t)q[2]], "output slot written twice or out of range");
      written[(size_t)q[2]] = 1;
      out[(size_t)q[2]] = acc[l];
    }
  }
  std::string line;
  std::vector<const int32_t*> entry(n_sets, nullptr);
  for (size_t k = 0; k < n_sets; k++) entry[(size_t)set_plan[MULTI_SET_WORDS * k + 2]] = set_plan + MULTI_SET_WORDS * k;
  for (size_t i = 0; i < n_sets; i++) {
    REQUIRE(written[i] && entry[i], "a set without a result");
    const int32_t* q = entry[i];
    const int pairs = 1 << q[3];
    REQUIRE(q[4] % pairs == 0 && q[4] / 32 == (q[4] + pairs - 1) / 32, "a set straddles a wave");
    REQUIRE(taken[i] == sets[i].items, "items added != the set's items: work does not follow the item count");
    uint32_t ncomp = 0;
    for (uint32_t c = 0; c < (uint32_t)q[1]; c++) ncomp += part_plan[MULTI_PART_WORDS * ((size_t)q[0] + c) + 3] & 1;
    char buf[128];
    snprintf(buf, sizeof buf, "%llu %d %d %u %u ", (unsigned long long)out[i], pairs, q[4], sets[i].items, ncomp);
    line += buf;
  }
  line += "P " + std::to_string(P.n_pairs) + " " + std::to_string(P.fold);
  return line;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: committeemulticheck CASES OUT");
  Input in;
  {
    std::ifstream f(argv[1]);
    REQUIRE(f.good(), "cannot read the case file");
    long long x;
    while (f >> x) in.v.push_back(x);
  }
  const size_t n_cases = (size_t)in.next();
  std::ofstream o(argv[2]);
  for (size_t k = 0; k < n_cases; k++) o << run_case(in) << "\n";
  REQUIRE(in.at == in.v.size(), "trailing integers in the case file");
  return 0;
}
