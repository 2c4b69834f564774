// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the fold of the signature MSM's bucket
// pass (lodestar_amd/csrc/lsg_curve.hpp g2_fold_mixed, the arithmetic of k_msm_bucket_seg) on the
// one-lane host build of the pair backend: the representation, bounds and lazy sums of the gfx950
// build.  A chunk is folded as the kernel folds it -- lane pair j of 2^ips_log2 takes members j,
// j + ips, ..., skips the ones that do not take part, lets the first one in as (x : y : 1) and adds
// the others by the mixed addition; then the pairs are combined by the kernel's butterfly, pair j
// adding pair j ^ o for o = ips / 2 .. 1 with the complete addition -- and beside it the same
// members are summed one after the other with the complete addition alone.
// tests/test_msm_buckets_host.py builds it plainly and with UBSan and compares both with the oracle.
//
//   bucketfoldcheck IN OUT
// IN: per chunk "C ips_log2 len", then per member "use" (0 / 1) and the affine point as signed
// decimal limbs, 14 per Fp value, x.c0 x.c1 y.c0 y.c1.
// OUT: per chunk one line: the fold's X Y Z, then the plain sum's X Y Z, in the same limb form.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
#include "lsg_pairing.hpp"

static int rd_fp(FILE* f, fp_t& a) {
  int got = 0;
  for (int k = 0; k < 14; k++) {
    long x;
    if (fscanf(f, "%ld", &x) == 1) {
      a.l[k] = (uint32_t)(int32_t)x;
      got++;
    }
  }
  return got == 14;
}
static int rd(FILE* f, fp2_t& a) { return rd_fp(f, a.c0) && rd_fp(f, a.c1); }
static void wr(FILE* f, const fp_t& a) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)a.l[k]);
}
static void wr(FILE* f, const g2p_t& p) {
  wr(f, p.X.c0);
  wr(f, p.X.c1);
  wr(f, p.Y.c0);
  wr(f, p.Y.c1);
  wr(f, p.Z.c0);
  wr(f, p.Z.c1);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: bucketfoldcheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "bucketfoldcheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  char op[8];
  while (fscanf(in, "%7s", op) == 1) {
    int ips_log2, len;
    if (strcmp(op, "C") || fscanf(in, "%d %d", &ips_log2, &len) != 2 || ips_log2 < 0 || ips_log2 > 5 || len < 0) {
      fprintf(stderr, "bucketfoldcheck: item %ld is malformed\n", item);
      return 2;
    }
    std::vector<g2a_t> pts((size_t)len);
    std::vector<int> use((size_t)len);
    for (int k = 0; k < len; k++)
      if (fscanf(in, "%d", &use[(size_t)k]) != 1 || !rd(in, pts[(size_t)k].x) || !rd(in, pts[(size_t)k].y)) {
        fprintf(stderr, "bucketfoldcheck: item %ld, member %d is malformed\n", item, k);
        return 2;
      }
    const int ips = 1 << ips_log2;
    std::vector<g2p_t> acc((size_t)ips);
    for (int j = 0; j < ips; j++)
      acc[(size_t)j] = g2_fold_mixed<fp2_t>(j, ips, len, [&](int k, g2a_t& a) {
        a = pts[(size_t)k];
        return use[(size_t)k] != 0;
      });
    for (int o = ips >> 1; o >= 1; o >>= 1) {
      const std::vector<g2p_t> before = acc;
      for (int j = 0; j < ips; j++) acc[(size_t)j] = g2_add(before[(size_t)j], before[(size_t)(j ^ o)]);
    }
    g2p_t plain = proj_inf<fp2_t>();
    for (int k = 0; k < len; k++)
      if (use[(size_t)k]) plain = g2_add(plain, proj_from_aff(pts[(size_t)k]));
    wr(out, acc[0]);
    wr(out, plain);
    fprintf(out, "\n");
    item++;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
