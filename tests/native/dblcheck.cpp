// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the doubling steps built on squares
// (lodestar_amd/csrc/lsg_curve.hpp proj_dbl, lsg_pairing.hpp ml_dbl_line_sq: the arithmetic of the
// fused Miller kernel's mf_dbl_line), of the scalar chains that use them (proj_mul_u64_s3:
// homogeneous throughout over Fp) and of the |x| chain with an affine base point (mixed additions),
// on the one-lane host build of the pair backend: the representation, bounds and lazy sums of the
// gfx950 build.  The reference side is a restatement, kept here, of the formulas these replaced
// (RCB 2016 algorithm 9 with 6 products and 3 squares; the window chain on Jacobian doublings with
// conversions around each complete addition), and for the Miller step the product's own
// ml_dbl_step_raw + line_eval, which keep the old formulas.
// tests/test_dbl_steps_host.py builds it plainly and with UBSan, and compares what it prints with
// each other, with Python integers and with the oracle.
//
//   dblcheck IN OUT
// IN: one item per line, an operation name and signed decimal limbs, 14 per Fp value (Fp2: c0
// then c1), a point as X Y Z:
//   D1 P            D2 P            proj_dbl over Fp / Fp2            -> new P', ref P'
//   L2 T xP yP                      the Miller doubling step          -> new (l00 l01 l11 X Y Z), ref
//   S1 P k          S2 P k          proj_mul_u64_s3 (k: decimal u64)  -> new P', ref P'
//   X2 x y                          [|x|](x, y) over Fp2              -> mixed P', full P', two flags
// OUT: per item one line of limbs in the same form (the flags of X2: g2_in_group_get with the
// affine and with the homogeneous getter).
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
#include "lsg_pairing.hpp"

// ---- the formulas these replaced
template <class F>
static proj_t<F> ref_proj_dbl(const proj_t<F>& p) {
  F t0 = fsqr(p.Y);
  F Z3 = fmulk<8>(t0);
  F t1 = fmul(p.Y, p.Z);
  F t2 = fmul_b3(fsqr(p.Z));
  F X3 = fmul(t2, Z3);
  F Y3 = fadd(t0, t2);
  Z3 = fmul(t1, Z3);
  t0 = fsub(t0, fmulk<3>(t2));
  Y3 = fmul(t0, Y3);
  Y3 = fadd(X3, Y3);
  t1 = fmul(p.X, p.Y);
  X3 = fmulk<2>(fmul(t0, t1));
  proj_t<F> r;
  r.X = X3;
  r.Y = Y3;
  r.Z = Z3;
  return r;
}
template <class F>
static proj_t<F> ref_mul_u64_s3(const proj_t<F>& p, uint64_t k) {
  const proj_t<F> T2 = ref_proj_dbl(p);
  const proj_t<F> T3 = proj_add(T2, p);
  const proj_t<F> T4 = ref_proj_dbl(T2);
  int d[22];
  unsigned c = 0;
  for (int i = 0; i < 22; i++) {
    int v = (int)((k >> (3 * i)) & 7u) + (int)c;
    c = (i < 21 && v >= 4) ? 1 : 0;
    d[i] = v - 8 * (int)c;
  }
  jac_t<F> acc = jac_from_proj(proj_pick_signed(p, T2, T3, T4, d[21]));
  for (int i = 20; i >= 0; i--) {
    for (int j = 0; j < 3; j++) acc = jac_dbl_t(acc);
    acc = jac_from_proj(proj_add(jac_to_proj(acc), proj_pick_signed(p, T2, T3, T4, d[i])));
  }
  return jac_to_proj(acc);
}

// ---- limb input and output
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
static int rd(FILE* f, fp_t& a) { return rd_fp(f, a); }
static int rd(FILE* f, fp2_t& a) { return rd_fp(f, a.c0) && rd_fp(f, a.c1); }
template <class F>
static int rd(FILE* f, proj_t<F>& p) {
  return rd(f, p.X) && rd(f, p.Y) && rd(f, p.Z);
}
static void wr(FILE* f, const fp_t& a) {
  for (int k = 0; k < 14; k++) fprintf(f, "%d ", (int32_t)a.l[k]);
}
static void wr(FILE* f, const fp2_t& a) {
  wr(f, a.c0);
  wr(f, a.c1);
}
template <class F>
static void wr(FILE* f, const proj_t<F>& p) {
  wr(f, p.X);
  wr(f, p.Y);
  wr(f, p.Z);
}

template <class F>
static int op_dbl(FILE* in, FILE* out) {
  proj_t<F> p;
  if (!rd(in, p)) return 0;
  wr(out, proj_dbl(p));
  wr(out, ref_proj_dbl(p));
  return 1;
}
template <class F>
static int op_s3(FILE* in, FILE* out) {
  proj_t<F> p;
  unsigned long long k;
  if (!rd(in, p) || fscanf(in, "%llu", &k) != 1) return 0;
  wr(out, proj_mul_u64_s3(p, (uint64_t)k));
  wr(out, ref_mul_u64_s3(p, (uint64_t)k));
  return 1;
}
static int op_line(FILE* in, FILE* out) {
  g2p_t T;
  g1a_t P;
  if (!rd(in, T) || !rd(in, P.x) || !rd(in, P.y)) return 0;
  fp2_t v[6];
  ml_dbl_line_sq<fp2_t>([&]() { return T; }, [&]() { return P; }, [](const fp_t& a) { return a; },
                        [&](int slot, const fp2_t& x) { v[slot] = x; });
  for (int j = 0; j < 6; j++) wr(out, v[j]);
  g2p_t R = T;
  const line_t L = line_eval(ml_dbl_step_raw(R), P.x, P.y);
  wr(out, L.l00);
  wr(out, L.l01);
  wr(out, L.l11);
  wr(out, R);
  return 1;
}
static int op_xabs(FILE* in, FILE* out) {
  g2a_t a;
  if (!rd(in, a.x) || !rd(in, a.y)) return 0;
  const g2p_t p = proj_from_aff(a);
  wr(out, proj_mul_xabs_get<fp2_t>([&]() { return a; }));
  wr(out, proj_mul_xabs_get<fp2_t>([&]() { return p; }));
  fprintf(out, "%d %d ", (int)g2_in_group_get<fp2_t>([&]() { return a; }), (int)g2_in_group_get<fp2_t>([&]() { return p; }));
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: dblcheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "dblcheck: cannot open files\n");
    return 2;
  }
  long item = 0;
  char op[8];
  while (fscanf(in, "%7s", op) == 1) {
    int ok;
    if (!strcmp(op, "D1"))
      ok = op_dbl<fp_t>(in, out);
    else if (!strcmp(op, "D2"))
      ok = op_dbl<fp2_t>(in, out);
    else if (!strcmp(op, "L2"))
      ok = op_line(in, out);
    else if (!strcmp(op, "S1"))
      ok = op_s3<fp_t>(in, out);
    else if (!strcmp(op, "S2"))
      ok = op_s3<fp2_t>(in, out);
    else if (!strcmp(op, "X2"))
      ok = op_xabs(in, out);
    else
      ok = 0;
    if (!ok) {
      fprintf(stderr, "dblcheck: item %ld (%s) is malformed\n", item, op);
      return 2;
    }
    fprintf(out, "\n");
    item++;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
