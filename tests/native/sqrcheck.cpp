// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the squaring leaves of
// lodestar_amd/csrc/lsg_fp_pair.hpp in the one-lane build (LSG_PAIR_G = 1: all 14 limbs in one
// "lane", the same representation and bounds as the gfx950 build).  tests/test_sqr_host.py
// builds it plainly and with UBSan and compares what it prints with Python integers.
//
//   sqrcheck IN OUT
// IN: one item per line, 28 signed decimal limbs (a0, a1).  OUT: per item one line of 42 limbs:
// pair_mont_sqr(a0), then c0 and c1 of the Fp2 squaring leaf on (a0, a1).  pair_mont_sqr(a0)
// is compared here, limb for limb, with pair_mont_mul(a0, a0): exit status 1 on a difference.
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

static void put(FILE* f, const fp_t& a) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)a.l[k]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sqrcheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "sqrcheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  for (;; item++) {
    fp_t a[2];
    int got = 0;
    for (int e = 0; e < 2; e++)
      for (int k = 0; k < 14; k++) {
        long v;
        if (fscanf(in, "%ld", &v) == 1) {
          a[e].l[k] = (uint32_t)(int32_t)v;
          got++;
        }
      }
    if (got == 0) break;
    if (got != 28) {
      fprintf(stderr, "sqrcheck: item %ld has %d limbs\n", item, got);
      return 2;
    }
    const fp_t s = pair_mont_sqr(a[0]), m = pair_mont_mul(a[0], a[0]);
    if (memcmp(s.l, m.l, sizeof s.l) != 0) {
      fprintf(stderr, "sqrcheck: item %ld: pair_mont_sqr differs from pair_mont_mul(a, a)\n", item);
      return 1;
    }
    const fp_duo q = pair_fp2_sqr(a[0], a[1]);
    put(out, s);
    put(out, q.x);
    put(out, q.y);
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
