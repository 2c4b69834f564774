// Fp2 with one COMPONENT per lane: the layout of the G2 [x] chains -- the whole chain of
// k_sig_subgroup (doublings, complete additions, the conversions around them) and the doublings
// of k_h2c_clear's two chains (its additions keep the pair form: lsg_k_hash.hip says why).
//
// An Fp2 element still takes one lane pair, but the even lane holds all 14 limbs of c0 and the
// odd lane all 14 limbs of c1 (fp2_t, lsg_tower.hpp, splits each component 7 + 7 over the pair).
// 14 words per lane either way; k_miller_fused (lsg_k_miller.hip) runs all four of its phases in
// this layout.  Each lane then runs a whole 14-column CIOS pass of its own:
//   product  every lane computes REDC(P b_own + Q b_other) with P = a0 on both lanes and
//            Q = -a1 on the even lane, a1 on the odd one: a0 b0 - a1 b1 | a0 b1 + a1 b0
//   square   the even lane computes REDC((a0 + a1)(a0 - a1)), the odd one REDC(a1 (2 a0))
//   by Fp    every lane computes REDC(a_own k), k's 14 limbs held by both lanes (fpv_t): the
//            line of the fused Miller kernel evaluated at P (lsg_k_miller.hip)
// so the per-step bookkeeping of the pair form (the m product and its broadcast, the 64-bit
// shift, the hand-down of lane 1's low limb, the b broadcasts) is paid once per 42 (28) mads
// instead of once per 14, the hand-down is gone, and b_own is a plain register read; b_other
// is one swap per step.  The mads are the same 588 (392) per lane.
//
// Limb convention of fp_t: a carried limb lies in [-8, 2^29 + 8], the top limb is signed, and
// |value| < 2^12.6 p.  The integers are those of the pair form at every operation: a carry round
// never changes the integer, a product returns (x + M p) / R with the M that x mod R fixes and
// leaves through a full normalisation, so a value converted back is word for word the pair
// form's.
//
// Column bound.  A lane holds a column for all 14 steps.  Per step a column takes
//   product: 3 terms (P b_own, Q b_other, m p), each below (2^29 + 8)^2 < 2^58.0001
//   square:  2 terms, the operand product below (2^30 + 16)(2^29 + 16) < 2^59.1 (the operands
//            a0 + a1, a0 - a1, 2 a0 are uncarried two-term sums) and m p below 2^58
//   by Fp:   2 terms, a_own k and m p, each below (2^29 + 8)^2 < 2^58.0001 (both operands are
//            carried values): inside the product's bound, on the square's pass (lanes_mul_pass)
// so after 7 steps |t| < 21 * 2^58.0001 < 2^62.4 (square: 7 (2^59.1 + 2^58) < 2^62.4).  The
// accumulators are carried once after step 7 (value-preserving: limbs back in [0, 2^29), the
// top one below 2^34 in magnitude) and the last 7 steps add the same again: |t| < 2^63
// throughout.  This is the mid-loop carry of the one-lane build of pair_sop2_n / pair_mont_mul_n.
// tests/test_fp2_lanes_model.py checks value, the m sequence and the bound at every step on
// Python integers; tests/native/fp2lanecheck.cpp runs the passes below under UBSan.
#pragma once

constexpr int LSG_VL = 14;  // limbs per lane

#if LSG_PAIR_G == 2
#define LSG_LANES_HIDE(x) asm volatile("" : "+v"(x))
#else
#define LSG_LANES_HIDE(x) ((void)0)
#endif

// ------------------------------------------------------------------ the pass of one lane
// (plain C++ on 14-word arrays: the device leaves below and the host driver run the same code)
LSG_PFN void lanes_carry64(int64_t* t) {
#pragma unroll
  for (int j = 0; j < LSG_VL - 1; j++) {
    t[j + 1] += t[j] >> 29;
    t[j] &= (int64_t)LSG_M29;
  }
}
// one reduction step: t += m p with m = -t[0] / p mod 2^29, then t >>= 29 (one column retires)
LSG_PFN void lanes_reduce_step(int64_t* t, const uint32_t* p, int i) {
  uint32_t m = ((uint32_t)t[0] * LSG_N0P) & LSG_M29;
  LSG_LANES_HIDE(m);
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) t[j] += (int64_t)(int32_t)m * (int32_t)p[j];
  const int64_t c = t[0] >> 29;
#pragma unroll
  for (int j = 0; j < LSG_VL - 1; j++) t[j] = t[j + 1];
  t[0] += c;
  t[LSG_VL - 1] = 0;
  if (i == 6) lanes_carry64(t);  // the mid-loop carry (see "Column bound" above)
}
// the end of the pass: limbs 0..12 in [0, 2^29), the signed top limb holds the rest
LSG_PFN void lanes_tail(int64_t* t, uint32_t* r) {
  lanes_carry64(t);
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) r[j] = (uint32_t)t[j];
}
// r = REDC(P b + Q other(b)): other(i, b[i]) is the partner lane's b[i]
template <class OTHER>
LSG_PFN void lanes_sop_pass(uint32_t* r, const uint32_t* P, const uint32_t* Q, const uint32_t* b, const OTHER& other) {
  uint32_t p[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) p[j] = LSG_P[j];
  int64_t t[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < LSG_VL; i++) {
    uint32_t bo = b[i], bs = other(i, b[i]);
    LSG_LANES_HIDE(bo);
    LSG_LANES_HIDE(bs);
#pragma unroll
    for (int j = 0; j < LSG_VL; j++) t[j] += (int64_t)(int32_t)P[j] * (int32_t)bo;
#pragma unroll
    for (int j = 0; j < LSG_VL; j++) t[j] += (int64_t)(int32_t)Q[j] * (int32_t)bs;
    lanes_reduce_step(t, p, i);
  }
  lanes_tail(t, r);
}
// r = REDC(V s)
LSG_PFN void lanes_mul_pass(uint32_t* r, const uint32_t* V, const uint32_t* s) {
  uint32_t p[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) p[j] = LSG_P[j];
  int64_t t[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < LSG_VL; i++) {
    uint32_t si = s[i];
    LSG_LANES_HIDE(si);
#pragma unroll
    for (int j = 0; j < LSG_VL; j++) t[j] += (int64_t)(int32_t)V[j] * (int32_t)si;
    lanes_reduce_step(t, p, i);
  }
  lanes_tail(t, r);
}
// r = REDC(a a), each cross product once.  At step i position j of the accumulators holds column
// i + j, so step i adds a_i a_i at position i and a_w (2 a_i) at every position w > i: 105 product
// mads for lanes_mul_pass's 196.  Every term of column c is added at a step <= c, so the column
// is complete when lanes_reduce_step retires it: the m sequence, and after lanes_tail the 14
// words, are those of lanes_mul_pass(r, a, a).  Per step a column takes one product term below
// (2^30 + 16)(2^29 + 8) < 2^59.1 and m p below 2^58: the square's bound above.
LSG_PFN void lanes_sqr_pass(uint32_t* r, const uint32_t* a) {
  uint32_t p[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) p[j] = LSG_P[j];
  int64_t t[LSG_VL];
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < LSG_VL; i++) {
    uint32_t ai = a[i], di = a[i] + a[i];
    LSG_LANES_HIDE(ai);
    LSG_LANES_HIDE(di);
    t[i] += (int64_t)(int32_t)a[i] * (int32_t)ai;
#pragma unroll
    for (int w = i + 1; w < LSG_VL; w++) t[w] += (int64_t)(int32_t)a[w] * (int32_t)di;
    lanes_reduce_step(t, p, i);
  }
  lanes_tail(t, r);
}

// ------------------------------------------------------------------ Fp with one ELEMENT per lane
// All 14 limbs of an Fp element on one lane and no cross-lane step at all: the layout of the
// fixed-exponent powers of k_fp_pow_lanes (lsg_k_reduce.hip), 64 elements per wave.  A product
// is lanes_mul_pass, a square lanes_sqr_pass; the integers are the pair form's at every step.
struct fpl_t {
  uint32_t l[LSG_VL];
};
LSG_PFN fpl_t lanes_fp_hide(fpl_t a) {  // (opaque operands: see lanes_fp2_mul_v)
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) LSG_LANES_HIDE(a.l[k]);
  return a;
}
LSG_PFN fpl_t lanes_fp_mul(const fpl_t& a, const fpl_t& b) {
  const fpl_t x = lanes_fp_hide(a), y = lanes_fp_hide(b);
  fpl_t r;
  lanes_mul_pass(r.l, x.l, y.l);
  return r;
}
LSG_PFN fpl_t lanes_fp_sqr(const fpl_t& a) {
  const fpl_t x = lanes_fp_hide(a);
  fpl_t r;
  lanes_sqr_pass(r.l, x.l);
  return r;
}
LSG_PFN fpl_t lanes_fp_select(bool c, const fpl_t& a, const fpl_t& b) {
  fpl_t r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = c ? a.l[k] : b.l[k];
  return r;
}
// a^e by the compile-time plan LSG_POW_PLANS[id] (lsg_fp_pair.hpp): pair_pow_plan's table, windows
// and loops, so the result is word for word pair_pow_plan(a, id).  id is wave-uniform.  The
// table is eight named values: as an array it went to scratch (464 bytes per lane).
#ifdef LSG_POW_IDS
LSG_PFN fpl_t lanes_pow_plan(const fpl_t& a, int id) {
  const pow_plan_t& P = LSG_POW_PLANS[id];
  const fpl_t a2 = lanes_fp_sqr(a);
  const fpl_t T0 = a;
  const fpl_t T1 = lanes_fp_mul(T0, a2);
  const fpl_t T2 = lanes_fp_mul(T1, a2);
  const fpl_t T3 = lanes_fp_mul(T2, a2);
  const fpl_t T4 = lanes_fp_mul(T3, a2);
  const fpl_t T5 = lanes_fp_mul(T4, a2);
  const fpl_t T6 = lanes_fp_mul(T5, a2);
  const fpl_t T7 = lanes_fp_mul(T6, a2);
  auto pick = [&](uint32_t k) {
    fpl_t tv = T0;
    tv = lanes_fp_select(k == 1u, T1, tv);
    tv = lanes_fp_select(k == 2u, T2, tv);
    tv = lanes_fp_select(k == 3u, T3, tv);
    tv = lanes_fp_select(k == 4u, T4, tv);
    tv = lanes_fp_select(k == 5u, T5, tv);
    tv = lanes_fp_select(k == 6u, T6, tv);
    tv = lanes_fp_select(k == 7u, T7, tv);
    return tv;
  };
  fpl_t r = pick(P.step[0] & 0xffu);
  const int n = P.n;
#pragma unroll 1
  for (int w = 1; w < n; w++) {
    const uint32_t s = P.step[w];
#pragma unroll 1
    for (uint32_t b = s >> 8; b; b--) r = lanes_fp_sqr(r);
    r = lanes_fp_mul(r, pick(s & 0xffu));
  }
#pragma unroll 1
  for (int b = P.tail; b; b--) r = lanes_fp_sqr(r);
  return r;
}
#endif
// An fp_t in the pair item-major layout (lane_store<fp_t>) is 14 consecutive words, limb 7 h + k
// at word 2 k + h: one lane reads or writes its element as seven 8-byte words.
LSG_PFN fpl_t lanes_fp_load(const uint32_t* mem, size_t i) {
  const uint32_t* w = mem + i * LSG_VL;
  fpl_t r;
#pragma unroll
  for (int k = 0; k < LSG_VL / 2; k++) {
    r.l[k] = w[2 * k];
    r.l[LSG_VL / 2 + k] = w[2 * k + 1];
  }
  return r;
}
LSG_PFN void lanes_fp_store(uint32_t* mem, size_t i, const fpl_t& a) {
  uint32_t* w = mem + i * LSG_VL;
#pragma unroll
  for (int k = 0; k < LSG_VL / 2; k++) {
    w[2 * k] = a.l[k];
    w[2 * k + 1] = a.l[LSG_VL / 2 + k];
  }
}

// The operands of a lane from its own word and its partner's (odd: the lane holds c1).
//   product: P = a0, Q = -a1 | a1        square: V = a0 + a1 | a1, s = a0 - a1 | 2 a0
//   by xi = 1 + u: a0 - a1 | a1 + a0 (a limb of the lazy sum, no pass)
LSG_PFN void lanes_mul_operand(uint32_t& P, uint32_t& Q, uint32_t own, uint32_t partner, bool odd) {
  P = odd ? partner : own;
  Q = odd ? own : 0u - partner;
}
LSG_PFN void lanes_sqr_operand(uint32_t& V, uint32_t& s, uint32_t own, uint32_t partner, bool odd) {
  V = odd ? own : own + partner;
  s = odd ? partner + partner : own - partner;
}
LSG_PFN uint32_t lanes_xi_operand(uint32_t own, uint32_t partner, bool odd) { return odd ? own + partner : own - partner; }

#if LSG_PAIR_G == 2
#define LSG_FP2_LANES 1
// ------------------------------------------------------------------ the type and its leaves
struct fp2v_t {
  uint32_t l[LSG_VL];  // even lane: c0, odd lane: c1
};
LSG_PFN bool lanes_odd() { return pair_h() != 0u; }
// the partner lane's word (quad_perm [1, 0, 3, 2]; every lane is written)
LSG_PFN uint32_t lanes_swap(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true);
}

// operands cross the leaf calls as vectors of 8 + 4 + 2 words (the call ABI passes vectors in
// VGPRs; two elements are 28 of the 31 argument registers)
typedef uint32_t lanes8_t __attribute__((ext_vector_type(8)));
typedef uint32_t lanes4_t __attribute__((ext_vector_type(4)));
typedef uint32_t lanes2_t __attribute__((ext_vector_type(2)));
#define LSG_LANES_PARAMS(x) lanes8_t x##_a, lanes4_t x##_b, lanes2_t x##_c
#define LSG_LANES_ARGS(v) lanes_pack8(v), lanes_pack4(v), lanes_pack2(v)
#define LSG_LANES_UNPACK(x) lanes_unpack(x##_a, x##_b, x##_c)
LSG_PFN lanes8_t lanes_pack8(const fp2v_t& a) {
  return lanes8_t{a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], a.l[6], a.l[7]};
}
LSG_PFN lanes4_t lanes_pack4(const fp2v_t& a) { return lanes4_t{a.l[8], a.l[9], a.l[10], a.l[11]}; }
LSG_PFN lanes2_t lanes_pack2(const fp2v_t& a) { return lanes2_t{a.l[12], a.l[13]}; }
LSG_PFN fp2v_t lanes_unpack(const lanes8_t& a, const lanes4_t& b, const lanes2_t& c) {
  fp2v_t r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.l[k] = a[k];
#pragma unroll
  for (int k = 0; k < 4; k++) r.l[8 + k] = b[k];
  r.l[12] = c[0];
  r.l[13] = c[1];
  return r;
}

LSG_PLEAF fp2v_t lanes_fp2_mul_v(LSG_LANES_PARAMS(va), LSG_LANES_PARAMS(vb)) {
  const fp2v_t a = LSG_LANES_UNPACK(va), b = LSG_LANES_UNPACK(vb);
  const bool odd = lanes_odd();
  uint32_t P[LSG_VL], Q[LSG_VL];
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) {
    lanes_mul_operand(P[k], Q[k], a.l[k], lanes_swap(a.l[k]), odd);
    // opaque operands: known non-negative limbs would turn the mads into v_mad_u64_u32 plus
    // accumulator moves (as in pair_pow_plan)
    LSG_LANES_HIDE(P[k]);
    LSG_LANES_HIDE(Q[k]);
  }
  fp2v_t r;
  lanes_sop_pass(r.l, P, Q, b.l, [](int, uint32_t x) { return lanes_swap(x); });
  return r;
}
LSG_PLEAF fp2v_t lanes_fp2_sqr_v(LSG_LANES_PARAMS(va)) {
  const fp2v_t a = LSG_LANES_UNPACK(va);
  const bool odd = lanes_odd();
  uint32_t V[LSG_VL], s[LSG_VL];
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) {
    lanes_sqr_operand(V[k], s[k], a.l[k], lanes_swap(a.l[k]), odd);
    LSG_LANES_HIDE(V[k]);
    LSG_LANES_HIDE(s[k]);
  }
  fp2v_t r;
  lanes_mul_pass(r.l, V, s);
  return r;
}

// An Fp element with all 14 limbs on both lanes of the pair: the Fp factor of the Fp2 x Fp leaf
struct fpv_t {
  uint32_t l[LSG_VL];
};
// a k = (a0 k) + (a1 k) u: one pass per lane on its own component, no cross-lane step
LSG_PLEAF fp2v_t lanes_fp2_mul_fp_v(LSG_LANES_PARAMS(va), LSG_LANES_PARAMS(vk)) {
  fp2v_t a = LSG_LANES_UNPACK(va), k = LSG_LANES_UNPACK(vk);
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) LSG_LANES_HIDE(a.l[j]);  // (opaque operands: see lanes_fp2_mul_v)
  fp2v_t r;
  lanes_mul_pass(r.l, a.l, k.l);
  return r;
}

// ------------------------------------------------------------------ conversions (DPP moves and selects)
// fp2_t: lane h holds limbs 7h..7h+6 of both components.  Each lane sends the 7 words its
// partner lacks (even: its half of c1, odd: its half of c0) in one swap per word.
LSG_PFN fp2v_t fp2v_from_pair(const fp2_t& a) {
  const bool odd = lanes_odd();
  fp2v_t r;
#pragma unroll
  for (int k = 0; k < LSG_PL; k++) {
    const uint32_t s = lanes_swap(odd ? a.c0.l[k] : a.c1.l[k]);
    r.l[k] = odd ? s : a.c0.l[k];
    r.l[LSG_PL + k] = odd ? a.c1.l[k] : s;
  }
  return r;
}
LSG_PFN fp2_t fp2v_to_pair(const fp2v_t& a) {
  const bool odd = lanes_odd();
  fp2_t r;
#pragma unroll
  for (int k = 0; k < LSG_PL; k++) {
    const uint32_t s = lanes_swap(odd ? a.l[k] : a.l[LSG_PL + k]);
    r.c0.l[k] = odd ? s : a.l[k];
    r.c1.l[k] = odd ? a.l[LSG_PL + k] : s;
  }
  return r;
}
// fp_t: lane h holds limbs 7h..7h+6.  Both lanes get all 14: 7 swaps and 14 selects.
LSG_PFN fpv_t fpv_from_pair(const fp_t& a) {
  const bool odd = lanes_odd();
  fpv_t r;
#pragma unroll
  for (int k = 0; k < LSG_PL; k++) {
    const uint32_t s = lanes_swap(a.l[k]);
    r.l[k] = odd ? s : a.l[k];
    r.l[LSG_PL + k] = odd ? a.l[k] : s;
  }
  return r;
}
LSG_PFN fp2v_t fp2v_from_const(const fpc_t& c0, const fpc_t& c1) {
  const bool odd = lanes_odd();
  fp2v_t r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = odd ? c1.l[k] : c0.l[k];
  return r;
}

// ------------------------------------------------------------------ linear operations
// Limb-wise on each lane's own component, no cross-lane step.  The lazy sums are those of
// lsg_fp_pair.hpp (fps_t<P, N>, the same bound rule and the same static_asserts): a lane's 14
// limbs carry like the pair's 7 + 7, without the word that crosses the pair.
LSG_PFN fp2v_t lanes_carry(const fp2v_t& a) {
  fp2v_t o;
  o.l[0] = a.l[0] & LSG_M29;
#pragma unroll
  for (int k = 1; k < LSG_VL - 1; k++) o.l[k] = (a.l[k] & LSG_M29) + (uint32_t)((int32_t)a.l[k - 1] >> 29);
  o.l[LSG_VL - 1] = a.l[LSG_VL - 1] + (uint32_t)((int32_t)a.l[LSG_VL - 2] >> 29);
  return o;
}
template <int P, int N>
struct fp2vs_t {
  uint32_t l[LSG_VL];
  LSG_PFN fp2v_t carry() const {
    static_assert(fps_carry_ok(P, N), "lazy sum too long for one carry round: carry a group first (P <= 3, N <= 3)");
    fp2v_t a;
#pragma unroll
    for (int k = 0; k < LSG_VL; k++) a.l[k] = l[k];
    return lanes_carry(a);
  }
  template <int K>
  LSG_PFN fp2v_t carry_mul() const {
    static_assert(fps_carry_mul_ok(K, P, N), "small multiple of this sum does not come out carried: carry() first");
    constexpr int m = fps_mulk_m(K), s = fps_mulk_s(K), sh = 29 - s;
    constexpr uint32_t lowm = (1u << sh) - 1;
    uint32_t t[LSG_VL];
#pragma unroll
    for (int k = 0; k < LSG_VL; k++) t[k] = m == 3 ? l[k] + (l[k] << 1) : l[k];
    fp2v_t o;
    o.l[0] = (t[0] & lowm) << s;
#pragma unroll
    for (int k = 1; k < LSG_VL - 1; k++) o.l[k] = ((t[k] & lowm) << s) + (uint32_t)((int32_t)t[k - 1] >> sh);
    o.l[LSG_VL - 1] = (t[LSG_VL - 1] << s) + (uint32_t)((int32_t)t[LSG_VL - 2] >> sh);
    return o;
  }
};
LSG_PFN fp2vs_t<1, 0> fsum(const fp2v_t& a) {
  fp2vs_t<1, 0> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = a.l[k];
  return r;
}
template <int P, int N, int Q, int M>
LSG_PFN fp2vs_t<P + Q, N + M> operator+(const fp2vs_t<P, N>& a, const fp2vs_t<Q, M>& b) {
  fp2vs_t<P + Q, N + M> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = a.l[k] + b.l[k];
  return r;
}
template <int P, int N, int Q, int M>
LSG_PFN fp2vs_t<P + M, N + Q> operator-(const fp2vs_t<P, N>& a, const fp2vs_t<Q, M>& b) {
  fp2vs_t<P + M, N + Q> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = a.l[k] - b.l[k];
  return r;
}
template <int P, int N>
LSG_PFN fp2vs_t<N, P> operator-(const fp2vs_t<P, N>& a) {
  fp2vs_t<N, P> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = 0u - a.l[k];
  return r;
}
template <int P, int N>
LSG_PFN fp2vs_t<P + 1, N> operator+(const fp2vs_t<P, N>& a, const fp2v_t& b) { return a + fsum(b); }
template <int P, int N>
LSG_PFN fp2vs_t<P, N + 1> operator-(const fp2vs_t<P, N>& a, const fp2v_t& b) { return a - fsum(b); }
template <int K, int P, int N>
LSG_PFN fp2vs_t<K * P, K * N> fsum_mulk(const fp2vs_t<P, N>& a) {
  static_assert(K >= 1 && K <= 3, "uncarried small multiples up to 3");
  fp2vs_t<K * P, K * N> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = a.l[k] * (uint32_t)K;
  return r;
}

// (1 + u) a = (c0 - c1) + (c0 + c1) u as a lazy sum: the even lane takes own - partner, the odd
// lane own + partner, one swap per limb.  The partner's sum has the same counts (P, N), so the
// even lane's result has (P + N, P + N) and the odd lane's (2 P, 2 N): the type keeps the larger.
constexpr int lanes_max(int a, int b) { return a > b ? a : b; }
template <int P, int N>
LSG_PFN fp2vs_t<lanes_max(P + N, 2 * P), lanes_max(P + N, 2 * N)> fsum_mul_xi(const fp2vs_t<P, N>& a) {
  const bool odd = lanes_odd();
  fp2vs_t<lanes_max(P + N, 2 * P), lanes_max(P + N, 2 * N)> r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = lanes_xi_operand(a.l[k], lanes_swap(a.l[k]), odd);
  return r;
}
LSG_PFN fp2vs_t<2, 1> fsum_mul_xi(const fp2v_t& a) { return fsum_mul_xi(fsum(a)); }

// ------------------------------------------------------------------ the generic names (lsg_curve.hpp)
LSG_PFN fp2v_t fmul(const fp2v_t& a, const fp2v_t& b) { return lanes_fp2_mul_v(LSG_LANES_ARGS(a), LSG_LANES_ARGS(b)); }
LSG_PFN fp2v_t fsqr(const fp2v_t& a) { return lanes_fp2_sqr_v(LSG_LANES_ARGS(a)); }
LSG_PFN fp2v_t fadd(const fp2v_t& a, const fp2v_t& b) { return (fsum(a) + b).carry(); }
LSG_PFN fp2v_t fsub(const fp2v_t& a, const fp2v_t& b) { return (fsum(a) - b).carry(); }
LSG_PFN fp2v_t fneg(const fp2v_t& a) { return (-fsum(a)).carry(); }
template <int K>
LSG_PFN fp2v_t fmulk(const fp2v_t& a) { return fsum(a).template carry_mul<K>(); }
// 12 (1 + u) a = 12 ((c0 - c1) + (c0 + c1) u): the one linear operation that crosses the pair.
// The even lane's a - partner is a sum of counts (1, 1), the odd lane's a + partner (2, 0):
// both inside (2, 1), carried, then 12 times a carried value in one pass (as fp2_mul_b3).
LSG_PFN fp2v_t fmul_b3(const fp2v_t& a) { return fmulk<12>(fsum_mul_xi(a).carry()); }
LSG_PFN fp2v_t fmul_xi(const fp2v_t& a) { return fsum_mul_xi(a).carry(); }
// (k goes through an fp2v_t to share the argument packing: the copy is gone after inlining)
LSG_PFN fp2v_t fmul_fp(const fp2v_t& a, const fpv_t& k) {
  fp2v_t kv;
#pragma unroll
  for (int j = 0; j < LSG_VL; j++) kv.l[j] = k.l[j];
  return lanes_fp2_mul_fp_v(LSG_LANES_ARGS(a), LSG_LANES_ARGS(kv));
}
LSG_PFN fp2v_t fselect(bool c, const fp2v_t& a, const fp2v_t& b) {  // c: the same on both lanes
  fp2v_t r;
#pragma unroll
  for (int k = 0; k < LSG_VL; k++) r.l[k] = c ? a.l[k] : b.l[k];
  return r;
}
// (a handful per item: through the pair form's canonical test)
LSG_PFN bool fis_zero(const fp2v_t& a) { return fp2_is_zero(fp2v_to_pair(a)); }

// ------------------------------------------------------------------ Fp6 = Fp2[v] / (v^3 - xi)
struct fp6v_t {
  fp2v_t c0, c1, c2;
};
LSG_PFN fp6v_t fp6_make(const fp2v_t& a, const fp2v_t& b, const fp2v_t& c) { return fp6v_t{a, b, c}; }
LSG_PFN fp6v_t fp6_add(const fp6v_t& a, const fp6v_t& b) {
  return fp6v_t{fadd(a.c0, b.c0), fadd(a.c1, b.c1), fadd(a.c2, b.c2)};
}
LSG_PFN fp6v_t fp6_mul_v(const fp6v_t& a) { return fp6v_t{fmul_xi(a.c2), a.c0, a.c1}; }
// the output coefficients of the Karatsuba Fp6 product as sums (lsg_tower.hpp fp6_kar_s0/1/2)
LSG_PFN fp2vs_t<3, 1> fp6_kar_s0(const fp2v_t& v0, const fp2v_t& v1, const fp2v_t& v2, const fp2v_t& m0) {
  return fsum(v0) + fsum_mul_xi((fsum(m0) - v1 - v2).carry());
}
LSG_PFN fp2vs_t<3, 3> fp6_kar_s1(const fp2v_t& v0, const fp2v_t& v1, const fp2v_t& v2, const fp2v_t& m1) {
  return (fsum(m1) - v0 - v1) + fsum_mul_xi(v2);
}
LSG_PFN fp2vs_t<2, 2> fp6_kar_s2(const fp2v_t& v0, const fp2v_t& v1, const fp2v_t& v2, const fp2v_t& m2) {
  return (fsum(m2) - v0 - v2) + v1;
}
#endif  // LSG_PAIR_G == 2
