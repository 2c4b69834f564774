// Optimal-ate Miller loop and final exponentiation for gfx950.  Replaces blst's
// miller_loop_n / final_exp used by Pairing.commit()/finalverify() under
// @chainsafe/blst verifyMultipleAggregateSignatures and verify
// (packages/beacon-node/src/chain/bls/maybeBatch.ts:18,37).
// Operation-for-operation mirror of oracle/pairing.py (dbl_step, add_step,
// f12_mul_line, miller_loop_fast, final_exp_fast), so per-pair Miller values are
// bit-comparable with the oracle.
#pragma once
#include "lsg_curve.hpp"

struct line_t {
  fp2_t l00, l01, l11;
};

// T <- 2T; returns the line unevaluated: (3b'Z^2 - Y^2, 3X^2, -2YZ); at P it is
// (l00, l01 xP, l11 yP) (line_eval)
LSG_BIGFN line_t ml_dbl_step_raw(g2p_t& T) {
  fp2_t t0 = fp2_sqr(T.Y);
  fp2_t t1 = fp2_mul(T.Y, T.Z);
  fp2_t t2 = fp2_mul_b3(fp2_sqr(T.Z));
  fp2_t XX = fp2_sqr(T.X);
  line_t L;
  L.l00 = fp2_sub(t2, t0);
  L.l01 = fp2_mulk<3>(XX);
  L.l11 = (-fp2s(t1)).carry_mul<2>();  // -2 t1
  fp2_t Z3 = fp2_mulk<8>(t0);
  fp2_t X3 = fp2_mul(t2, Z3);
  fp2_t Y3 = fp2_add(t0, t2);
  Z3 = fp2_mul(t1, Z3);
  fp2_t s0 = (fp2s(t0) - fp2s_mulk<3>(fp2s(t2))).carry();  // t0 - 3 t2
  Y3 = fp2_mul(s0, Y3);
  Y3 = fp2_add(X3, Y3);
  fp2_t v1 = fp2_mul(T.X, T.Y);
  X3 = fp2_mulk<2>(fp2_mul(s0, v1));
  T.X = X3;
  T.Y = Y3;
  T.Z = Z3;
  return L;
}

// T <- T + Q; theta = Y - yQ Z, delta = X - xQ Z; unevaluated line (delta yQ - theta xQ,
// theta, -delta); at P: (l00, theta xP, -delta yP)
LSG_BIGFN line_t ml_add_step_raw(g2p_t& T, g2a_t Q) {
  fp2_t theta = fp2_sub(T.Y, fp2_mul(Q.y, T.Z));
  fp2_t delta = fp2_sub(T.X, fp2_mul(Q.x, T.Z));
  line_t L;
  L.l00 = fp2_sub(fp2_mul(delta, Q.y), fp2_mul(theta, Q.x));
  L.l01 = theta;
  L.l11 = fp2_neg(delta);
  fp2_t C = fp2_sqr(theta);
  fp2_t D = fp2_sqr(delta);
  fp2_t E = fp2_mul(D, delta);
  fp2_t F = fp2_mul(T.Z, C);
  fp2_t G = fp2_mul(T.X, D);
  fp2_t H = (fp2s(E) + F - fp2s_mulk<2>(fp2s(G))).carry();  // E + F - 2G: one carry
  fp2_t X3 = fp2_mul(delta, H);
  fp2_t Y3 = fp2_sub(fp2_mul(theta, fp2_sub(G, H)), fp2_mul(E, T.Y));
  fp2_t Z3 = fp2_mul(E, T.Z);
  T.X = X3;
  T.Y = Y3;
  T.Z = Z3;
  return L;
}

// an unevaluated line at the G1 point P = (xP, yP)
LSG_INL line_t line_eval(line_t L, const fp_t& xP, const fp_t& yP) {
  L.l01 = fp2_mul_fp(L.l01, xP);
  L.l11 = fp2_mul_fp(L.l11, yP);
  return L;
}

// The doubling step of the fused Miller kernel (lsg_k_miller.hip mf_dbl_line): the field elements
// of ml_dbl_step_raw + line_eval from 2 products and 7 squares (there: 6 and 3), over either Fp2
// layout F.  With B = Y^2, C = Z^2, J = X^2, E = 3b' C:
//   2YZ = (Y + Z)^2 - B - C,   2XY = (X + Y)^2 - J - B,
//   X3 = (B - 3E) 2XY,   Z3 = 4B 2YZ,   Y3 = (B + 3E)^2 - 12 E^2  (= (B - 3E)(B + E) + 8 B E);
//   the line at P is (E - B, 3J xP, 2YZ (-yP)), the sign of its last coefficient taken on yP.
// getT() gives T, getP() the G1 point (read late: after the squares), fp_in(a) an Fp value in the
// form F's product by Fp takes.  put(slot, v) receives each value as soon as it exists: slots
// 0..2 the line's coefficients, 3..5 the new X, Y, Z -- in the order Z, X, Y.
template <class F, class GetT, class GetP, class FpIn, class Put>
LSG_INL void ml_dbl_line_sq(const GetT& getT, const GetP& getP, const FpIn& fp_in, const Put& put) {
  F B, E, yz2, xy2;
  {
    const proj_t<F> T = getT();
    B = fsqr(T.Y);
    const F C = fsqr(T.Z);
    yz2 = fsub2(fsqr(fadd(T.Y, T.Z)), B, C);
    E = fmul_b3(C);
    const F J = fsqr(T.X);
    xy2 = fsub2(fsqr(fadd(T.X, T.Y)), J, B);
    const g1a_t Pk = getP();
    put(0, fsub(E, B));
    put(1, fmul_fp(fmulk<3>(J), fp_in(Pk.x)));
    put(2, fmul_fp(yz2, fp_in(fp_neg(Pk.y))));
  }
  put(5, fmul(fmulk<4>(B), yz2));
  const F s0 = (fsum(B) - fsum_mulk<3>(fsum(E))).carry();  // B - 3E
  put(3, fmul(s0, xy2));
  const F s1 = (fsum_mulk<2>(fsum(B)) - s0).carry();  // B + 3E = 2B - (B - 3E)
  put(4, fsub(fsqr(s1), fmulk<12>(fsqr(E))));
}

// ---- Output combinations of the fused Miller kernel's phases (lsg_k_miller.hip: mf_sqr,
// mf_pair_lines, mf_mul_pair), as functions of the phase's Fp2 products V(p).  Each output
// coefficient is one linear combination of up to 11 products and their xi multiples; written
// as lazy sums they are regrouped so that every carry takes a group of at most three added
// and three subtracted values (the type rule): 2-5 carry rounds per component where the
// nested fp2_add / fp2_sub form paid 6-14.  Regrouping an integer linear combination does not
// change its value, so each result is the integer of the nested form (tests/native/sumcheck.cpp
// holds those forms and compares).
// S phase, f <- f^2: V0..5 the Karatsuba products of t = a b, V6..11 those of
// u = (a + b)(a + v b).  J = 0..2: new c1.J = 2 t_J;  J = 3..5: new c0.(J-3) = (u - t - v t)_(J-3).
// The products come in the layout V returns them in (fp2_t, or fp2v_t of lsg_fp2_lanes.hpp whose
// sums count the larger of the two lanes' terms): every grouping below fits both.
template <int J, class G>
LSG_INL auto mfc_sqr(const G& V) {
  if constexpr (J == 0) {
    return fp6_kar_s0(V(0), V(1), V(2), V(3)).template carry_mul<2>();
  } else if constexpr (J == 1) {
    return fp6_kar_s1(V(0), V(1), V(2), V(4)).template carry_mul<2>();
  } else if constexpr (J == 2) {
    return fp6_kar_s2(V(0), V(1), V(2), V(5)).template carry_mul<2>();
  } else if constexpr (J == 3) {  // u0 - t0 - xi t2 = V6 - V0 + xi ((m0' - v1' - v2') - (m0 - v1 - v2) - t2)
    const auto e = ((fsum(V(9)) - V(7) - V(8)) - (fsum(V(3)) - V(1) - V(2))).carry();
    const auto g = (fsum(e) - fp6_kar_s2(V(0), V(1), V(2), V(5))).carry();
    return (fsum(V(6)) - V(0) + fsum_mul_xi(g)).carry();
  } else if constexpr (J == 4) {  // u1 - t1 - t0, with u1 - t1 = (m1' - v0' - v1') - (m1 - v0 - v1) + xi (v2' - v2)
    const auto d = ((fsum(V(10)) - V(6) - V(7)) - (fsum(V(4)) - V(0) - V(1))).carry();
    const auto e = (fsum(d) + fsum_mul_xi(fsum(V(8)) - V(2))).carry();
    return (fsum(e) - fp6_kar_s0(V(0), V(1), V(2), V(3))).carry();
  } else {  // u2 - t2 - t1, with u2 - t2 = (m2' - v0' - v2') - (m2 - v0 - v2) + v1' - v1
    const auto d = ((fsum(V(11)) - V(6) - V(8)) - (fsum(V(5)) - V(0) - V(2))).carry();
    const auto t1 = fp6_kar_s1(V(0), V(1), V(2), V(4)).carry();
    return (fsum(d) + V(7) - V(1) - t1).carry();
  }
}
// P phase, M = l l' of two sparse lines from P0..P5 = V(0..5) (see mf_pair_lines):
// J = 0: m0 = P0 + xi P1, 1: m1 = P3 - P0 - P2, 2: m4 = P4 - P0 - P1, 3: m5 = P5 - P2 - P1
template <int J, class G>
LSG_INL auto mfc_pair(const G& V) {
  if constexpr (J == 0) {
    return (fsum(V(0)) + fsum_mul_xi(V(1))).carry();
  } else if constexpr (J == 1) {
    return fsub2(V(3), V(0), V(2));
  } else if constexpr (J == 2) {
    return fsub2(V(4), V(0), V(1));
  } else {
    return fsub2(V(5), V(2), V(1));
  }
}
// M phase, f <- f M from V0..16 (see mf_mul_pair): t0 = a M0 from V0..5 (m0 = V4, m1 = V3,
// m2 = V5), n = b (m4 + m5 v): n0 = V6 + xi V10, n1 = V8 - V6 - V7, n2 = V7 + V9, t2 = s q from
// V11..16 (m0 = V15, m1 = V14, m2 = V16).  J = 0..2: f'.c0.J = (t0 + v (v n))_J, i.e.
// t0_0 + xi n1, t0_1 + xi n2, t0_2 + n0;  J = 3..5: f'.c1.(J-3) = (t2 - t0 - v n)_(J-3), i.e.
// t2_0 - t0_0 - xi n2, t2_1 - t0_1 - n0, t2_2 - t0_2 - n1.
template <int J, class G>
LSG_INL auto mfc_mul(const G& V) {
  if constexpr (J == 0) {  // V0 + xi (V4 - V1 - V2 + V8 - V6 - V7)
    const auto g = (fsum(V(4)) - V(1) - V(2) + V(8)).carry();
    const auto h = (fsum(g) - V(6) - V(7)).carry();
    return (fsum(V(0)) + fsum_mul_xi(h)).carry();
  } else if constexpr (J == 1) {  // V3 - V0 - V1 + xi (V2 + V7 + V9)
    const auto h = (fsum(V(2)) + V(7) + V(9)).carry();
    return ((fsum(V(3)) - V(0) - V(1)) + fsum_mul_xi(h)).carry();
  } else if constexpr (J == 2) {  // V5 - V0 - V2 + V1 + V6 + xi V10
    const auto n0 = (fsum(V(6)) + fsum_mul_xi(V(10))).carry();
    return (fsum(V(5)) - V(0) - V(2) + V(1) + n0).carry();
  } else if constexpr (J == 3) {  // V11 - V0 + xi (V15 - V12 - V13 - V4 + V1 + V2 - V7 - V9)
    const auto g = (fsum(V(15)) - V(12) - V(13) + V(1) + V(2)).carry();
    const auto h = (fsum(g) - V(4) - V(7) - V(9)).carry();
    return (fsum(V(11)) - V(0) + fsum_mul_xi(h)).carry();
  } else if constexpr (J == 4) {  // (V14 - V11 - V12) - (V3 - V0 - V1) - V6 + xi (V13 - V2 - V10)
    const auto a = ((fsum(V(14)) - V(11) - V(12)) - (fsum(V(3)) - V(0) - V(1))).carry();
    const auto b = fsub2(V(13), V(2), V(10));
    return (fsum(a) - V(6) + fsum_mul_xi(b)).carry();
  } else {  // V16 + V12 + V0 + V2 + V6 + V7 - V11 - V13 - V5 - V1 - V8
    const auto g = (fsum(V(11)) + V(13) + V(5) - V(16) - V(12) - V(0)).carry();
    return (fsum(V(2)) + V(6) + V(7) - V(1) - V(8) - g).carry();
  }
}

// T <- 2T; line = (3b'Z^2 - Y^2, 3X^2 xP, -2YZ yP)
LSG_INL line_t ml_dbl_step(g2p_t& T, fp_t xP, fp_t yP) { return line_eval(ml_dbl_step_raw(T), xP, yP); }

// T <- T + Q; line = (delta yQ - theta xQ, theta xP, -delta yP)
LSG_INL line_t ml_add_step(g2p_t& T, g2a_t Q, fp_t xP, fp_t yP) {
  return line_eval(ml_add_step_raw(T, Q), xP, yP);
}

// f_{|x|,Q}(P) conjugated (x < 0).  P affine G1, Q affine G2, both finite.
LSG_BIGFN fp12_t miller_loop(g1a_t P, g2a_t Q) {
  const uint64_t xa = ((uint64_t)LSG_X_ABS_HI << 32) | LSG_X_ABS_LO;
  g2p_t T = proj_from_aff(Q);
  line_t L = ml_dbl_step(T, P.x, P.y);
  fp12_t f;
  f.c0 = fp6_make(L.l00, L.l01, fp2_zero());
  f.c1 = fp6_make(fp2_zero(), L.l11, fp2_zero());
  // bit 62 of |x| is 1
  L = ml_add_step(T, Q, P.x, P.y);
  f = fp12_mul_line(f, L.l00, L.l01, L.l11);
  for (int b = 61; b >= 0; b--) {
    f = fp12_sqr(f);
    L = ml_dbl_step(T, P.x, P.y);
    f = fp12_mul_line(f, L.l00, L.l01, L.l11);
    if ((xa >> b) & 1u) {
      L = ml_add_step(T, Q, P.x, P.y);
      f = fp12_mul_line(f, L.l00, L.l01, L.l11);
    }
  }
  return fp12_conj(f);
}

LSG_INL fp12_t fp12_from_line(const line_t& L) {
  fp12_t f;
  f.c0 = fp6_make(L.l00, L.l01, fp2_zero());
  f.c1 = fp6_make(fp2_zero(), L.l11, fp2_zero());
  return f;
}
LSG_INL fp12_t fp12_select(bool c, const fp12_t& a, const fp12_t& b) {
  fp12_t r;
  r.c0 = fp6_make(fp2_select(c, a.c0.c0, b.c0.c0), fp2_select(c, a.c0.c1, b.c0.c1), fp2_select(c, a.c0.c2, b.c0.c2));
  r.c1 = fp6_make(fp2_select(c, a.c1.c0, b.c1.c0), fp2_select(c, a.c1.c1, b.c1.c1), fp2_select(c, a.c1.c2, b.c1.c2));
  return r;
}

// Multi-Miller loop over K pairs sharing one f and its squarings (blst miller_loop_n):
// returns prod_{k: use[k]} conj(f_{|x|,Q_k}(P_k)), the same field element as the product of
// the per-pair miller_loop() values.  Pairs with use[k] == false contribute 1 (their point
// arithmetic still runs so that every row of a wave follows one control path).
template <int K>
LSG_INL fp12_t miller_loop_multi(const g1a_t (&P)[K], const g2a_t (&Q)[K], const bool (&use)[K]) {
  const uint64_t xa = ((uint64_t)LSG_X_ABS_HI << 32) | LSG_X_ABS_LO;
  g2p_t T[K];
  fp12_t f = fp12_one();
  bool started = false;  // row-uniform: f still 1
#pragma unroll
  for (int k = 0; k < K; k++) {
    T[k] = proj_from_aff(Q[k]);
    line_t L = ml_dbl_step(T[k], P[k].x, P[k].y);
    fp12_t g = started ? fp12_mul_line(f, L.l00, L.l01, L.l11) : fp12_from_line(L);
    f = fp12_select(use[k], g, f);
    started = true;
  }
#pragma unroll
  for (int k = 0; k < K; k++) {  // bit 62 of |x| is 1
    line_t L = ml_add_step(T[k], Q[k], P[k].x, P[k].y);
    f = fp12_select(use[k], fp12_mul_line(f, L.l00, L.l01, L.l11), f);
  }
#pragma unroll 1
  for (int b = 61; b >= 0; b--) {
    f = fp12_sqr(f);
#pragma unroll
    for (int k = 0; k < K; k++) {
      line_t L = ml_dbl_step(T[k], P[k].x, P[k].y);
      f = fp12_select(use[k], fp12_mul_line(f, L.l00, L.l01, L.l11), f);
    }
    if ((xa >> b) & 1u) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        line_t L = ml_add_step(T[k], Q[k], P[k].x, P[k].y);
        f = fp12_select(use[k], fp12_mul_line(f, L.l00, L.l01, L.l11), f);
      }
    }
  }
  return fp12_conj(f);
}

// ---- Split Miller loop (device path): the G2 side and the Fp12 side run as two kernels.
// miller_lines writes the ML_STEPS unevaluated lines of one Q in loop order (step 0: the
// first doubling, step 1: the addition for bit 62, then per bit b = 61..0 a doubling and,
// for set bits, an addition); miller_accum_multi evaluates them at the P_k and accumulates
// f with the same operation order as miller_loop_multi, so the result is the same field
// element.  Each kernel then holds only its own half of the state (T and a line, or f and a
// line) instead of f, K points and the line together.
constexpr int ML_STEPS = 68;  // 63 doublings + 5 additions for |x| = 0xd201000000010000

template <class Put>
LSG_INL void miller_lines(const g2a_t& Q, Put&& put) {
  const uint64_t xa = ((uint64_t)LSG_X_ABS_HI << 32) | LSG_X_ABS_LO;
  g2p_t T = proj_from_aff(Q);
  int s = 0;
  put(s++, ml_dbl_step_raw(T));
  put(s++, ml_add_step_raw(T, Q));
#pragma unroll 1
  for (int b = 61; b >= 0; b--) {
    put(s++, ml_dbl_step_raw(T));
    if ((xa >> b) & 1u) put(s++, ml_add_step_raw(T, Q));
  }
}

// get(k, step) -> the unevaluated line of pair k at that step
template <int K, class Get>
LSG_INL fp12_t miller_accum_multi(const g1a_t (&P)[K], const bool (&use)[K], Get&& get) {
  const uint64_t xa = ((uint64_t)LSG_X_ABS_HI << 32) | LSG_X_ABS_LO;
  fp12_t f = fp12_one();
#pragma unroll
  for (int k = 0; k < K; k++) {
    line_t L = line_eval(get(k, 0), P[k].x, P[k].y);
    fp12_t g = k > 0 ? fp12_mul_line(f, L.l00, L.l01, L.l11) : fp12_from_line(L);
    f = fp12_select(use[k], g, f);
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    line_t L = line_eval(get(k, 1), P[k].x, P[k].y);
    f = fp12_select(use[k], fp12_mul_line(f, L.l00, L.l01, L.l11), f);
  }
  int s = 2;
#pragma unroll 1
  for (int b = 61; b >= 0; b--) {
    f = fp12_sqr(f);
    const int n_steps = 1 + (int)((xa >> b) & 1u);
#pragma unroll 1
    for (int j = 0; j < n_steps; j++, s++) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        line_t L = line_eval(get(k, s), P[k].x, P[k].y);
        f = fp12_select(use[k], fp12_mul_line(f, L.l00, L.l01, L.l11), f);
      }
    }
  }
  return fp12_conj(f);
}

// g^x for g in the cyclotomic subgroup
LSG_BIGFN fp12_t fp12_exp_by_x(fp12_t g) {
  const uint64_t xa = ((uint64_t)LSG_X_ABS_HI << 32) | LSG_X_ABS_LO;
  fp12_t r = g;
  for (int b = 62; b >= 0; b--) {
    r = fp12_cyclotomic_sqr(r);
    if ((xa >> b) & 1u) r = fp12_mul(r, g);
  }
  return fp12_conj(r);
}

// f^(3 (p^12 - 1)/r)   -- oracle/pairing.py:final_exp_fast
LSG_BIGFN fp12_t final_exp(fp12_t f) {
  fp12_t f1 = fp12_mul(fp12_conj(f), fp12_inv(f));
  fp12_t g = fp12_mul(fp12_frob2(f1), f1);
  fp12_t t0 = fp12_mul(fp12_exp_by_x(g), fp12_conj(g));
  t0 = fp12_mul(fp12_exp_by_x(t0), fp12_conj(t0));
  fp12_t t1 = fp12_mul(fp12_exp_by_x(t0), fp12_frob(t0));
  fp12_t t2 = fp12_mul(fp12_mul(fp12_exp_by_x(fp12_exp_by_x(t1)), fp12_frob2(t1)), fp12_conj(t1));
  return fp12_mul(t2, fp12_mul(fp12_sqr(g), g));
}
