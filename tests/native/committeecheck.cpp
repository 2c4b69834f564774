// committeecheck.cpp -- CPU driver of the committee + bits policy in lodestar_amd/csrc/lsg_plan.hpp
// and of the bit walk in lsg_bits.h (tests/test_committee_plan_host.py).  No device: committee
// members are small integers standing in for keys, "addition" is addition mod the prime
// 2^61 - 1, the identity is 0.  Each case's sets are staged (bits_stage_set), planned
// (plan_bits) and then executed as k_pk_agg_bits executes them: per lane pair the walk over
// the staged field, the fold, the butterfly over the set's pairs within its wave, the
// complement against the committee sum.
//
//   committeecheck CASES OUT    CASES: whitespace-separated integers, OUT: one line per case
//
// CASES = n_cases, then per case  n_sets, per set:
//   len member[len]  n_bits  n_bytes byte[n_bytes]      (n_bytes >= ceil(n_bits / 8))
// OUT per case: per set "result complement pairs first_pair wanted", then "P n_pairs fold".
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
  fprintf(stderr, "committeecheck: %s\n", m.c_str());
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

std::string run_case(Input& in) {
  const size_t n_sets = (size_t)in.next();
  // the committee store: every set's committee registered under its own id
  std::vector<uint32_t> cm_off(n_sets);
  std::vector<uint64_t> cm_rows, cm_sum(n_sets, 0);
  std::vector<std::vector<uint8_t>> fields(n_sets);
  std::vector<uint32_t> n_bits(n_sets);
  size_t words = 0;
  for (size_t i = 0; i < n_sets; i++) {
    const size_t len = (size_t)in.next();
    cm_off[i] = (uint32_t)cm_rows.size();
    for (size_t k = 0; k < len; k++) {
      const uint64_t m = (uint64_t)in.next();
      cm_rows.push_back(m);
      cm_sum[i] = add(cm_sum[i], m);
    }
    n_bits[i] = (uint32_t)in.next();
    REQUIRE(n_bits[i] == len, "a set's bit count is its committee's length");
    const size_t nb = (size_t)in.next();
    REQUIRE(nb >= (n_bits[i] + 7) / 8, "bitfield shorter than n_bits");
    fields[i].resize(nb);
    for (size_t k = 0; k < nb; k++) fields[i][k] = (uint8_t)in.next();
    words += bits_words(n_bits[i]);
  }
  // staging, exactly sized: a write past a set's words is an AddressSanitizer report
  std::vector<uint32_t> arena(words);
  std::vector<BitsSet> sets;
  size_t bw = 0;
  for (size_t i = 0; i < n_sets; i++)
    sets.push_back(bits_stage_set((uint32_t)i, fields[i].data(), n_bits[i], (int32_t)i, arena.data(), &bw));
  REQUIRE(bw <= words, "arena overrun");
  std::vector<int32_t> A;
  A.push_back(12345);  // (the plan does not start at word 0 of its arena)
  const BitsPlan P = plan_bits(A, sets);
  REQUIRE(P.n_sets == n_sets, "one plan entry per set");
  const int32_t* plan = A.data() + P.plan_off;
  const int32_t* pair_set = A.data() + P.pair_off;
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
      const int32_t* q = plan + BITS_PLAN_WORDS * (size_t)e[l];
      const uint32_t cid = (uint32_t)q[0], nb = (uint32_t)q[2];
      const uint32_t* field = arena.data() + (uint32_t)q[1];
      const bool complement = (q[3] & 1) != 0;
      ips[l] = 1 << (q[3] >> 8);
      j[l] = (int)item - q[5];
      REQUIRE(j[l] >= 0 && j[l] < ips[l], "pair outside its set's range");
      if (!nb) continue;
      REQUIRE((size_t)q[1] + bits_words(nb) <= arena.size(), "field outside the arena");
      const uint32_t inv = complement ? ~0u : 0u;
      lsg_bits_walk wk = lsg_bits_begin(field, nb, inv, (uint32_t)j[l]);
      for (int32_t m = lsg_bits_next(field, nb, inv, (uint32_t)ips[l], wk); m >= 0;
           m = lsg_bits_next(field, nb, inv, (uint32_t)ips[l], wk)) {
        REQUIRE((uint32_t)m < nb, "walk left the field");
        acc[l] = add(acc[l], cm_rows[cm_off[cid] + (uint32_t)m]);
        taken[(size_t)q[4]]++;
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
      const int32_t* q = plan + BITS_PLAN_WORDS * (size_t)e[l];
      if (q[3] & 1) acc[l] = add(cm_sum[(uint32_t)q[0]], neg(acc[l]));
      REQUIRE(q[4] >= 0 && (size_t)q[4] < n_sets && !written[(size_t)q[4]], "output slot written twice or out of range");
      written[(size_t)q[4]] = 1;
      out[(size_t)q[4]] = acc[l];
    }
  }
  std::string line;
  std::vector<const int32_t*> entry(n_sets, nullptr);
  for (size_t k = 0; k < n_sets; k++) entry[(size_t)plan[BITS_PLAN_WORDS * k + 4]] = plan + BITS_PLAN_WORDS * k;
  for (size_t i = 0; i < n_sets; i++) {
    REQUIRE(written[i] && entry[i], "a set without a result");
    const int32_t* q = entry[i];
    const int pairs = 1 << (q[3] >> 8);
    REQUIRE(pairs <= 32, "more pairs than a wave holds");
    REQUIRE(q[5] % pairs == 0 && q[5] / 32 == (q[5] + pairs - 1) / 32, "a set straddles a wave");
    const uint32_t wanted = sets[i].n_bits ? bits_wanted(sets[i].n_bits, sets[i].p) : 0;
    REQUIRE(taken[i] == wanted, "members added != wanted members: work does not follow the wanted count");
    char buf[128];
    snprintf(buf, sizeof buf, "%llu %d %d %d %u ", (unsigned long long)out[i], q[3] & 1, pairs, q[5], wanted);
    line += buf;
  }
  line += "P " + std::to_string(P.n_pairs) + " " + std::to_string(P.fold);
  return line;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: committeecheck CASES OUT");
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
