// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the per-lane passes of
// lodestar_amd/csrc/lsg_fp2_lanes.hpp (the Fp2 layout with one component per lane): the code
// each gfx950 lane runs, with the partner lane simulated here -- lane 0 holds the 14 limbs of c0,
// lane 1 those of c1, and a "swap" reads the other lane's array.  tests/test_fp2_lanes_host.py
// builds it plainly and with UBSan (a column overflow of the 64-bit accumulators traps) and
// compares what it prints with Python integers and the oracle.
//
//   fp2lanecheck IN OUT
// IN: one item per line, 56 signed decimal limbs (a0, a1, b0, b1).  OUT: per item one line of 56
// limbs: lanes 0 and 1 of the product a b, then lanes 0 and 1 of the square of a.
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

// what lanes_fp2_mul_v does on lane `lane` of the pair (a[h], b[h]: the words lane h holds)
static __attribute__((noinline)) void lane_mul(uint32_t* r, const uint32_t a[2][14], const uint32_t b[2][14], int lane) {
  uint32_t P[14], Q[14];
  for (int k = 0; k < 14; k++) lanes_mul_operand(P[k], Q[k], a[lane][k], a[lane ^ 1][k], lane != 0);
  const uint32_t* partner = b[lane ^ 1];
  lanes_sop_pass(r, P, Q, b[lane], [partner](int i, uint32_t) { return partner[i]; });
}
// ... and lanes_fp2_sqr_v
static __attribute__((noinline)) void lane_sqr(uint32_t* r, const uint32_t a[2][14], int lane) {
  uint32_t V[14], s[14];
  for (int k = 0; k < 14; k++) lanes_sqr_operand(V[k], s[k], a[lane][k], a[lane ^ 1][k], lane != 0);
  lanes_mul_pass(r, V, s);
}

static void put(FILE* f, const uint32_t* l) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)l[k]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: fp2lanecheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "fp2lanecheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  for (;; item++) {
    uint32_t v[4][14];
    int got = 0;
    for (int e = 0; e < 4; e++)
      for (int k = 0; k < 14; k++) {
        long x;
        if (fscanf(in, "%ld", &x) == 1) {
          v[e][k] = (uint32_t)(int32_t)x;
          got++;
        }
      }
    if (got == 0) break;
    if (got != 56) {
      fprintf(stderr, "fp2lanecheck: item %ld has %d limbs\n", item, got);
      return 2;
    }
    uint32_t r[14];
    for (int lane = 0; lane < 2; lane++) {
      lane_mul(r, &v[0], &v[2], lane);
      put(out, r);
    }
    for (int lane = 0; lane < 2; lane++) {
      lane_sqr(r, &v[0], lane);
      put(out, r);
    }
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
