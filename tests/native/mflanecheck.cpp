// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the two per-lane operations the fused
// Miller kernel adds to lodestar_amd/csrc/lsg_fp2_lanes.hpp (the Fp2 layout with one component
// per lane): the Fp2 x Fp product (lanes_fp2_mul_fp_v: one lanes_mul_pass per lane, the Fp factor
// on both lanes) and the product by xi = 1 + u as a lazy sum (fsum_mul_xi: lanes_xi_operand per
// limb).  The code each gfx950 lane runs, with the partner lane simulated here as in
// fp2lanecheck.cpp -- lane 0 holds the 14 limbs of c0, lane 1 those of c1.
// lane_xi restates fsum_mul_xi's loop over lanes_xi_operand (the device function reads its partner
// with a DPP swap, which the host cannot run): the operand choice is checked here, the swap and the
// selection on the device by lsg_check_mf_lanes (tests/test_gpu_miller_lanes.py).
// tests/test_miller_lanes_host.py builds it plainly and with UBSan and compares what it prints
// with Python integers and the oracle.
//
//   mflanecheck IN OUT
// IN: one item per line, 42 signed decimal limbs (a0, a1, k).  OUT: per item one line of 56
// limbs: lanes 0 and 1 of a k, then lanes 0 and 1 of the uncarried sum xi a.
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

// what lanes_fp2_mul_fp_v does on lane `lane` of the pair (a[h]: the words lane h holds)
static __attribute__((noinline)) void lane_mul_fp(uint32_t* r, const uint32_t a[2][14], const uint32_t* k, int lane) {
  lanes_mul_pass(r, a[lane], k);
}
// ... and fsum_mul_xi
static __attribute__((noinline)) void lane_xi(uint32_t* r, const uint32_t a[2][14], int lane) {
  for (int k = 0; k < 14; k++) r[k] = lanes_xi_operand(a[lane][k], a[lane ^ 1][k], lane != 0);
}

static void put(FILE* f, const uint32_t* l) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)l[k]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mflanecheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "mflanecheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  for (;; item++) {
    uint32_t v[3][14];
    int got = 0;
    for (int e = 0; e < 3; e++)
      for (int k = 0; k < 14; k++) {
        long x;
        if (fscanf(in, "%ld", &x) == 1) {
          v[e][k] = (uint32_t)(int32_t)x;
          got++;
        }
      }
    if (got == 0) break;
    if (got != 42) {
      fprintf(stderr, "mflanecheck: item %ld has %d limbs\n", item, got);
      return 2;
    }
    uint32_t r[14];
    for (int lane = 0; lane < 2; lane++) {
      lane_mul_fp(r, &v[0], v[2], lane);
      put(out, r);
    }
    for (int lane = 0; lane < 2; lane++) {
      lane_xi(r, &v[0], lane);
      put(out, r);
    }
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
