// lsg_bits.h -- the walk over a participation bitfield that k_pk_agg_bits (lsg_k_pk.hip) runs
// on the device and tests/native/committeecheck.cpp runs on the CPU: one text for both, so the
// CPU test executes what the kernel executes.  Plain integers only.
//
// A staged bitfield is ceil(n_bits / 32) little-endian words: member k is bit k & 31 of word
// k >> 5 (the bytes of an SSZ bitvector copied as they are: bit k & 7 of byte k >> 3).  The
// WANTED members of a set are its set bits (direct mode, inv = 0) or its clear bits below
// n_bits (complement mode, inv = ~0); bits at positions >= n_bits are never wanted, whatever
// the padding holds.  The wanted members are dealt to the set's lane pairs round robin by
// rank: pair j of `stride` takes the wanted members of rank j, j + stride, ...  Whole words
// are skipped by population count, so a pair's work follows the number of members it takes
// plus the number of words, not the committee length.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LSG_HD __host__ __device__ inline
#else
#define LSG_HD inline
#endif

// words per set in the plan of k_pk_agg_bits (lsg_plan.hpp plan_bits)
#define LSG_BITS_PLAN_WORDS 6

// word k (< ceil(n_bits / 32)) of the wanted mask
LSG_HD uint32_t lsg_bits_word(const uint32_t* bits, uint32_t k, uint32_t n_bits, uint32_t inv) {
  uint32_t w = bits[k] ^ inv;
  const uint32_t left = n_bits - 32u * k;
  if (left < 32u) w &= (1u << left) - 1u;
  return w;
}

struct lsg_bits_walk {
  uint32_t k;     // current word
  uint32_t w;     // its wanted bits not yet passed
  uint32_t skip;  // wanted members to pass over before the next one taken
};

// pair j's walk over a field of n_bits >= 1 bits
LSG_HD lsg_bits_walk lsg_bits_begin(const uint32_t* bits, uint32_t n_bits, uint32_t inv, uint32_t j) {
  lsg_bits_walk s;
  s.k = 0;
  s.w = lsg_bits_word(bits, 0, n_bits, inv);
  s.skip = j;
  return s;
}

// the next member this pair takes, or -1 when the field is exhausted
LSG_HD int32_t lsg_bits_next(const uint32_t* bits, uint32_t n_bits, uint32_t inv, uint32_t stride, lsg_bits_walk& s) {
  const uint32_t n_words = (n_bits + 31u) >> 5;
  for (;;) {
    const uint32_t c = (uint32_t)__builtin_popcount(s.w);
    if (s.skip >= c) {
      s.skip -= c;
      if (++s.k >= n_words) {
        s.k = n_words;
        s.w = 0;
        return -1;
      }
      s.w = lsg_bits_word(bits, s.k, n_bits, inv);
      continue;
    }
    for (; s.skip; s.skip--) s.w &= s.w - 1u;
    const int32_t m = (int32_t)(32u * s.k) + __builtin_ctz(s.w);
    s.w &= s.w - 1u;
    s.skip = stride - 1u;
    return m;
  }
}

// ---- a set spanning several committees (LSG_PK_BITS_MULTI; k_pk_agg_bits_multi): its parts,
// one per listed committee with a wanted member or a stored sum to add, each with its own
// word-aligned field and mode.  Plan words (lsg_plan.hpp plan_multi):
//   per set:  first part, part count (0: write the identity), output slot, pairs log2, first pair
//   per part: committee id, arena word, n_bits (>= 1), mode (bit 0: complement)
#define LSG_MULTI_SET_WORDS 5
#define LSG_MULTI_PART_WORDS 4

// Pair j's walk over the wanted members of parts [0, n_parts) of one set, dealt round robin by
// their rank ACROSS the parts: the skip count left over when a part's walk ends carries into
// the next part's lsg_bits_begin.
struct lsg_multi_walk {
  uint32_t c;       // current part
  uint32_t open;    // its walk has begun
  uint32_t skip;    // carried into the next part
  lsg_bits_walk w;
};

LSG_HD lsg_multi_walk lsg_multi_begin(uint32_t j) {
  lsg_multi_walk s;
  s.c = 0;
  s.open = 0;
  s.skip = j;
  s.w.k = s.w.w = s.w.skip = 0;
  return s;
}

// the next member this pair takes: its index in part s.c (parts: that set's part records), or
// -1 when every part is exhausted
LSG_HD int32_t lsg_multi_next(const int32_t* parts, uint32_t n_parts, const uint32_t* bits, uint32_t stride,
                              lsg_multi_walk& s) {
  for (; s.c < n_parts; s.c++, s.open = 0) {
    const int32_t* q = parts + LSG_MULTI_PART_WORDS * s.c;
    const uint32_t* field = bits + (uint32_t)q[1];
    const uint32_t n_bits = (uint32_t)q[2], inv = (q[3] & 1) ? ~0u : 0u;
    if (!s.open) {
      s.w = lsg_bits_begin(field, n_bits, inv, s.skip);
      s.open = 1;
    }
    const int32_t m = lsg_bits_next(field, n_bits, inv, stride, s.w);
    if (m >= 0) return m;
    s.skip = s.w.skip;
  }
  return -1;
}
