// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the lazy sums of
// lodestar_amd/csrc/lsg_fp_pair.hpp and of every formula rewritten with them (lsg_tower.hpp,
// lsg_curve.hpp, lsg_pairing.hpp), in the one-lane build (LSG_PAIR_G = 1: all 14 limbs in one
// "lane", the same representation and bounds as the gfx950 build).  tests/test_sums_host.py builds
// it lazily, with -DLSG_EAGER_SUMS (every operation carried: the formulas as they were), with
// UBSan and with -DLSG_SUM_AUDIT, runs each build directly and compares the integers they print.
//
//   sumcheck IN OUT
// IN: one item per line, 28 signed decimal limbs (two elements).  The elements of all items form
// one ring; item i works on the elements that follow its own.  OUT: per item one line of 14-limb
// groups in the order of the emit() calls below; the first HEAVY items add the scalar chains,
// the cofactor clearing and the Miller loops.
// The output combinations of the fused Miller kernel (mfc_sqr, mfc_pair, mfc_mul) are compared
// here, as integers, with the nested fp2_add / fp2_sub forms they replaced: exit status 1 on a
// difference.
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
#include "lsg_h2c.hpp"
#include "lsg_pairing.hpp"

static const int HEAVY = 6;
static std::vector<fp_t> ring;
static FILE* out;

static void emit(const fp_t& a) {
  for (int k = 0; k < 14; k++) fprintf(out, "%d ", (int32_t)a.l[k]);
}
static void emit(const fp2_t& a) {
  emit(a.c0);
  emit(a.c1);
}
static void emit(const fp6_t& a) {
  emit(a.c0);
  emit(a.c1);
  emit(a.c2);
}
static void emit(const fp12_t& a) {
  emit(a.c0);
  emit(a.c1);
}
template <class F>
static void emit(const proj_t<F>& p) {
  emit(p.X);
  emit(p.Y);
  emit(p.Z);
}
template <class F>
static void emit(const jac_t<F>& p) {
  emit(p.X);
  emit(p.Y);
  emit(p.Z);
}
static void emit(const line_t& L) {
  emit(L.l00);
  emit(L.l01);
  emit(L.l11);
}

// the same integer?  (pair_full_norm is value-preserving and its limbs are unique)
static bool same_int(const fp_t& a, const fp_t& b) {
  const fp_t x = pair_full_norm(a), y = pair_full_norm(b);
  return memcmp(x.l, y.l, sizeof x.l) == 0;
}
static bool same_int(const fp2_t& a, const fp2_t& b) { return same_int(a.c0, b.c0) && same_int(a.c1, b.c1); }

// ---- the nested forms of the fused kernel's combinations, as they stood before the lazy sums
template <class G>
static fp2_t ref_fin(const G& V, int base, int j) {
  const fp2_t v0 = V(base), v1 = V(base + 1), v2 = V(base + 2);
  if (j == 0) return fp2_add(v0, fp2_mul_xi(fp2_sub(fp2_sub(V(base + 3), v1), v2)));
  if (j == 1) return fp2_add(fp2_sub(fp2_sub(V(base + 4), v0), v1), fp2_mul_xi(v2));
  return fp2_add(fp2_sub(fp2_sub(V(base + 5), v0), v2), v1);
}
template <class G>
static fp2_t ref_sqr(const G& V, int J) {
  if (J < 3) {
    const fp2_t o = ref_fin(V, 0, J);
    return fp2_add(o, o);
  }
  if (J == 3) return fp2_sub(fp2_sub(ref_fin(V, 6, 0), ref_fin(V, 0, 0)), fp2_mul_xi(ref_fin(V, 0, 2)));
  if (J == 4) return fp2_sub(fp2_sub(ref_fin(V, 6, 1), ref_fin(V, 0, 1)), ref_fin(V, 0, 0));
  return fp2_sub(fp2_sub(ref_fin(V, 6, 2), ref_fin(V, 0, 2)), ref_fin(V, 0, 1));
}
template <class G>
static fp2_t ref_pair(const G& V, int J) {
  if (J == 0) return fp2_add(V(0), fp2_mul_xi(V(1)));
  if (J == 1) return fp2_sub(fp2_sub(V(3), V(0)), V(2));
  if (J == 2) return fp2_sub(fp2_sub(V(4), V(0)), V(1));
  return fp2_sub(fp2_sub(V(5), V(2)), V(1));
}
template <class G>
static fp2_t ref_mul(const G& V, int J) {
  auto t0c = [&](int j) {
    if (j == 0) return fp2_add(V(0), fp2_mul_xi(fp2_sub(fp2_sub(V(4), V(1)), V(2))));
    if (j == 1) return fp2_add(fp2_sub(fp2_sub(V(3), V(0)), V(1)), fp2_mul_xi(V(2)));
    return fp2_add(fp2_sub(fp2_sub(V(5), V(0)), V(2)), V(1));
  };
  auto t2c = [&](int j) {
    if (j == 0) return fp2_add(V(11), fp2_mul_xi(fp2_sub(fp2_sub(V(15), V(12)), V(13))));
    if (j == 1) return fp2_add(fp2_sub(fp2_sub(V(14), V(11)), V(12)), fp2_mul_xi(V(13)));
    return fp2_add(fp2_sub(fp2_sub(V(16), V(11)), V(13)), V(12));
  };
  auto nc = [&](int j) {
    if (j == 0) return fp2_add(V(6), fp2_mul_xi(V(10)));
    if (j == 1) return fp2_sub(fp2_sub(V(8), V(6)), V(7));
    return fp2_add(V(7), V(9));
  };
  if (J == 0) return fp2_add(t0c(0), fp2_mul_xi(nc(1)));
  if (J == 1) return fp2_add(t0c(1), fp2_mul_xi(nc(2)));
  if (J == 2) return fp2_add(t0c(2), nc(0));
  if (J == 3) return fp2_sub(fp2_sub(t2c(0), t0c(0)), fp2_mul_xi(nc(2)));
  if (J == 4) return fp2_sub(fp2_sub(t2c(1), t0c(1)), nc(0));
  return fp2_sub(fp2_sub(t2c(2), t0c(2)), nc(1));
}

static long item_no;
static void check(bool ok, const char* what, int j) {
  if (!ok) {
    fprintf(stderr, "sumcheck: item %ld: %s<%d> differs from the nested form\n", item_no, what, j);
    exit(1);
  }
}
template <int J, class G>
static void do_sqr(const G& V) {
  const fp2_t r = mfc_sqr<J>(V);
  check(same_int(r, ref_sqr(V, J)), "mfc_sqr", J);
  emit(r);
}
template <int J, class G>
static void do_pair(const G& V) {
  const fp2_t r = mfc_pair<J>(V);
  check(same_int(r, ref_pair(V, J)), "mfc_pair", J);
  emit(r);
}
template <int J, class G>
static void do_mul(const G& V) {
  const fp2_t r = mfc_mul<J>(V);
  check(same_int(r, ref_mul(V, J)), "mfc_mul", J);
  emit(r);
}

static void light(size_t i) {
  const size_t n = ring.size();
  auto E = [&](size_t j) { return ring[(2 * i + j) % n]; };
  auto E2 = [&](size_t j) { return fp2_t(E(2 * j), E(2 * j + 1)); };
  const fp_t a = E(0), b = E(1), c = E(2), d = E(3), e = E(4), f = E(5);
  // 0: the maximal admissible chain; 1..5: the small multiples; 6..8: carried multiples of sums
  emit((fps(a) + b + c - d - e - f).carry());
  emit(fp_mulk<2>(a));
  emit(fp_mulk<3>(a));
  emit(fp_mulk<4>(a));
  emit(fp_mulk<8>(a));
  emit(fp_mulk<12>(a));
  emit((fps(a) + b + c - d - e - f).carry_mul<2>());
  emit((fps(a) + b + c - d).carry_mul<4>());
  emit((fps(a) + b).carry_mul<8>());
  // 9..: (-a - b - c + d).carry(), then the Fp2 primitives
  emit((-(fps(a) + b + c) + d).carry());
  emit(fp2_mul_xi(E2(0)));
  emit(fp2_mul_b3(E2(0)));
  emit(fp_mul12(a));
  emit((fp2s_conj(fp2s(E2(0)) - E2(1)) + fp2s_mul_xi(E2(2))).carry());
  // the tower
  const fp6_t x6 = fp6_make(E2(0), E2(1), E2(2)), y6 = fp6_make(E2(3), E2(4), E2(5));
  const fp12_t x12 = fp12_make(x6, y6), y12 = fp12_make(fp6_make(E2(6), E2(7), E2(8)), fp6_make(E2(9), E2(10), E2(11)));
  emit(fp6_mul(x6, y6));
  emit(fp6_mul_01(x6, E2(6), E2(7)));
  emit(fp12_mul(x12, y12));
  emit(fp12_sqr(x12));
  emit(fp12_mul<false>(x12, y12));
  emit(fp12_sqr<false>(x12));
  emit(fp12_mul_line(x12, E2(12), E2(13), E2(14)));
  {
    fp2_t c0, c1;
    fp4_square(c0, c1, E2(0), E2(1));
    emit(c0);
    emit(c1);
  }
  // the curve
  const jac_t<fp_t> j1 = {a, b, c};
  const jac_t<fp2_t> j2 = {E2(0), E2(1), E2(2)};
  emit(jac_dbl(j1));
  emit(jac_dbl(j2));
  const g1p_t p1 = {a, b, c}, q1 = {d, e, f};
  const g2p_t p2 = {E2(0), E2(1), E2(2)}, q2 = {E2(3), E2(4), E2(5)};
  emit(g1_dbl(p1));
  emit(g2_dbl(p2));
  emit(g1_add(p1, q1));
  emit(g2_add(p2, q2));
  emit(g1_add_mixed(p1, g1a_t{d, e}));
  emit(g2_add_mixed(p2, g2a_t{E2(3), E2(4)}));
  // the Miller steps
  {
    g2p_t T = p2;
    emit(ml_dbl_step_raw(T));
    emit(T);
    T = p2;
    emit(ml_add_step_raw(T, g2a_t{E2(3), E2(4)}));
    emit(T);
  }
  // the fused kernel's combinations (checked against the nested forms above)
  auto V = [&](int p) { return E2((size_t)p + 1); };
  do_sqr<0>(V);
  do_sqr<1>(V);
  do_sqr<2>(V);
  do_sqr<3>(V);
  do_sqr<4>(V);
  do_sqr<5>(V);
  do_pair<0>(V);
  do_pair<1>(V);
  do_pair<2>(V);
  do_pair<3>(V);
  do_mul<0>(V);
  do_mul<1>(V);
  do_mul<2>(V);
  do_mul<3>(V);
  do_mul<4>(V);
  do_mul<5>(V);
}

// whole chains on tamed operands (|v| < 2p, as the kernels' inputs are)
static void heavy(size_t i) {
  const size_t n = ring.size();
  auto T = [&](size_t j) { return fp_tame(ring[(2 * i + j) % n]); };
  auto T2 = [&](size_t j) { return fp2_t(T(2 * j), T(2 * j + 1)); };
  const g1p_t p1 = {T(0), T(1), T(2)};
  const g2p_t p2 = {T2(0), T2(1), T2(2)};
  emit(proj_mul_u64_s3(p1, 0x9e3779b97f4a7c15ull + (uint64_t)i * 0x0123456789abcdefull));
  emit(proj_mul_xabs<fp2_t>(p2));
  emit(clear_cofactor_g2(p2));
  const g1a_t P[2] = {{T(0), T(1)}, {T(6), T(7)}};
  const g2a_t Q[2] = {{T2(1), T2(2)}, {T2(4), T2(5)}};
  emit(miller_loop(P[0], Q[0]));
  // the split loop on two pairs: lines first, then the accumulation with shared squarings
  static line_t lines[2][ML_STEPS];
  for (int k = 0; k < 2; k++) miller_lines(Q[k], [&](int st, const line_t& L) { lines[k][st] = L; });
  const bool use[2] = {true, true};
  emit(miller_accum_multi<2>(P, use, [&](int k, int st) { return lines[k][st]; }));
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sumcheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "sumcheck: cannot open files\n");
    return 2;
  }
  for (;;) {
    fp_t a;
    int got = 0;
    for (int k = 0; k < 14; k++) {
      long v;
      if (fscanf(in, "%ld", &v) == 1) {
        a.l[k] = (uint32_t)(int32_t)v;
        got++;
      }
    }
    if (got == 0) break;
    if (got != 14) {
      fprintf(stderr, "sumcheck: element %zu has %d limbs\n", ring.size(), got);
      return 2;
    }
    ring.push_back(a);
  }
  fclose(in);
  if (ring.size() < 2 || ring.size() % 2) {
    fprintf(stderr, "sumcheck: %zu elements\n", ring.size());
    return 2;
  }
  const size_t items = ring.size() / 2;
  for (size_t i = 0; i < items; i++) {
    item_no = (long)i;
    light(i);
    if (i < (size_t)HEAVY) heavy(i);
    fprintf(out, "\n");
  }
  if (fclose(out) != 0) return 2;
  printf("%zu\n", items);
  return 0;
}
