// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the one-element-per-lane squaring pass
// and fixed-exponent power of lodestar_amd/csrc/lsg_fp2_lanes.hpp (lanes_sqr_pass,
// lanes_pow_plan: the code each gfx950 lane of k_fp_pow_lanes runs) beside the one-lane host
// build of the pair form (pair_pow_plan, LSG_PAIR_G = 1).  tests/test_fp_pow_lanes_host.py builds
// it plainly and with UBSan (a column overflow of the 64-bit accumulators traps) and compares
// what it prints with Python integers and the oracle's field.
//
//   powlanecheck IN OUT
// IN: one element per line, 14 signed decimal limbs.  OUT: per element one line of 56 limbs: the
// square, then the powers for the plan ids 0, 1, 2.  The driver itself checks, word for word,
// that lanes_sqr_pass(a) is lanes_mul_pass(a, a) and that lanes_pow_plan is pair_pow_plan, and
// exits with status 1 at the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#define __noinline__ __attribute__((noinline))
#endif

#define LSG_PAIR_G 1
#include "lsg_fp_pair.hpp"
#include "lsg_fp2_lanes.hpp"

static __attribute__((noinline)) void lane_sqr(uint32_t* r, const uint32_t* a) { lanes_sqr_pass(r, a); }
static __attribute__((noinline)) void lane_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) { lanes_mul_pass(r, a, b); }
static __attribute__((noinline)) fpl_t lane_pow(const fpl_t& a, int id) { return lanes_pow_plan(a, id); }

static void put(FILE* f, const uint32_t* l) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)l[k]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: powlanecheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "powlanecheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  for (;; item++) {
    fpl_t a;
    int got = 0;
    for (int k = 0; k < 14; k++) {
      long x;
      if (fscanf(in, "%ld", &x) == 1) {
        a.l[k] = (uint32_t)(int32_t)x;
        got++;
      }
    }
    if (got == 0) break;
    if (got != 14) {
      fprintf(stderr, "powlanecheck: item %ld has %d limbs\n", item, got);
      return 2;
    }
    uint32_t s[14], m[14];
    lane_sqr(s, a.l);
    lane_mul(m, a.l, a.l);
    if (memcmp(s, m, sizeof s) != 0) {
      fprintf(stderr, "powlanecheck: item %ld: lanes_sqr_pass differs from lanes_mul_pass(a, a)\n", item);
      return 1;
    }
    put(out, s);
    fp_t pa;
    for (int k = 0; k < 14; k++) pa.l[k] = a.l[k];
    for (int id = 0; id < 3; id++) {
      const fpl_t r = lane_pow(a, id);
      const fp_t q = pair_pow_plan(pa, id);
      if (memcmp(r.l, q.l, sizeof r.l) != 0) {
        fprintf(stderr, "powlanecheck: item %ld: lanes_pow_plan differs from pair_pow_plan, id %d\n", item, id);
        return 1;
      }
      put(out, r.l);
    }
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
