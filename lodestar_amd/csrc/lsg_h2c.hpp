// hash_to_G2 for gfx950: RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_ as used by blst's
// Pairing(hash_or_encode = true, DST) inside @chainsafe/blst verifyMultipleAggregateSignatures
// (reached from packages/beacon-node/src/chain/bls/maybeBatch.ts:18,37).
//   expand_message_xmd (SHA-256) -> hash_to_field (4 Fp) -> simplified SWU on E2'
//   -> 3-isogeny -> Q0 + Q1 -> clear_cofactor (psi form) .
// Mirrors oracle/hash_to_curve.py step for step.
#pragma once
#include "lsg_curve.hpp"

// SHA-256 (SHA_K, sha256_compress, be_words_to_bytes) and the SSZ signing roots built on it
// (the variable-size kinds call their node hash instead of inlining it thirty times)
#define LSG_SSZ_CALL __device__ __noinline__
#include "lsg_ssz.hpp"
#ifdef LSG_SSZ_CALL_DEFAULTED
#error "lsg_ssz.hpp was included before lsg_h2c.hpp: its functions are the host program's, not the device's"
#endif

// Streaming SHA-256 over bytes (messages here are < 2^32 bits).
struct sha256_ctx {
  uint32_t st[8];
  uint32_t blk[16];
  uint32_t n;      // bytes in current block
  uint32_t total;  // total bytes
};

LSG_INL void sha256_init(sha256_ctx& c) {
  c.st[0] = 0x6a09e667u;
  c.st[1] = 0xbb67ae85u;
  c.st[2] = 0x3c6ef372u;
  c.st[3] = 0xa54ff53au;
  c.st[4] = 0x510e527fu;
  c.st[5] = 0x9b05688cu;
  c.st[6] = 0x1f83d9abu;
  c.st[7] = 0x5be0cd19u;
  for (int i = 0; i < 16; i++) c.blk[i] = 0;
  c.n = 0;
  c.total = 0;
}

LSG_INL void sha256_byte(sha256_ctx& c, uint8_t v) {
  uint32_t wi = c.n >> 2, sh = 24 - 8 * (c.n & 3);
  c.blk[wi] |= (uint32_t)v << sh;
  c.n++;
  c.total++;
  if (c.n == 64) {
    sha256_compress(c.st, c.blk);
    for (int i = 0; i < 16; i++) c.blk[i] = 0;
    c.n = 0;
  }
}

LSG_INL void sha256_bytes(sha256_ctx& c, const uint8_t* p, uint32_t len) {
  for (uint32_t i = 0; i < len; i++) sha256_byte(c, p[i]);
}

LSG_INL void sha256_final(sha256_ctx& c, uint32_t* out8) {
  uint32_t bits = c.total * 8;
  sha256_byte(c, 0x80);
  while (c.n != 56) sha256_byte(c, 0);
  c.blk[14] = 0;
  c.blk[15] = bits;
  sha256_compress(c.st, c.blk);
  for (int i = 0; i < 8; i++) out8[i] = c.st[i];
}

// expand_message_xmd(msg, DST, 256) -> 256 bytes   (RFC 9380 section 5.3.1)
LSG_INL void expand_message_xmd_256(uint8_t* out, const uint8_t* msg, uint32_t msg_len, const uint8_t* dst,
                                    uint32_t dst_len) {
  sha256_ctx c;
  uint32_t b0[8], bi[8];
  sha256_init(c);
  for (int i = 0; i < 64; i++) sha256_byte(c, 0);  // Z_pad
  sha256_bytes(c, msg, msg_len);
  sha256_byte(c, 1);  // l_i_b_str = 256 (2 bytes, big endian)
  sha256_byte(c, 0);
  sha256_byte(c, 0);  // I2OSP(0, 1)
  sha256_bytes(c, dst, dst_len);
  sha256_byte(c, (uint8_t)dst_len);
  sha256_final(c, b0);
  for (int i = 1; i <= 8; i++) {
    sha256_init(c);
    for (int k = 0; k < 8; k++) {
      uint32_t v = (i == 1) ? b0[k] : (b0[k] ^ bi[k]);
      sha256_byte(c, (uint8_t)(v >> 24));
      sha256_byte(c, (uint8_t)(v >> 16));
      sha256_byte(c, (uint8_t)(v >> 8));
      sha256_byte(c, (uint8_t)v);
    }
    sha256_byte(c, (uint8_t)i);
    sha256_bytes(c, dst, dst_len);
    sha256_byte(c, (uint8_t)dst_len);
    sha256_final(c, bi);
    be_words_to_bytes(out + 32 * (i - 1), bi, 8);
  }
}

// 64 big-endian bytes -> element mod p, Montgomery form.  Split N into three pieces that
// are each < p (a Montgomery product needs both inputs < p):
//   N = hi * 2^384 + mid * 2^256 + lo,  hi, mid < 2^128, lo < 2^256
//   mont(N) = mont_mul(lo, R^2) + mont_mul(mid, 2^256 R^2) + mont_mul(hi, R^3)
LSG_INL fp_t fp_from_be64_mod(const uint8_t* b) {
  fp_t lo = fp_from_be_bytes(b + 32, 8);
  fp_t mid = fp_from_be_bytes(b + 16, 4);
  fp_t hi = fp_from_be_bytes(b, 4);
  return fp_add(fp_add(fp_mul(lo, fp_t(FP_R2)), fp_mul(mid, fp_t(FP_R2_SHL256))), fp_mul(hi, fp_t(FP_R3)));
}

// ------------------------------------------------------------------ SSWU on E2' (RFC 9380 6.6.2)
// One exponentiation decides between x1 and x2 for every row of the wave at once (no
// divergent second square root): with gx2 = (Z u^2)^3 gx1 and N(Z) = 5 a non-square in Fp,
// if N(gx1) is a non-square then
//   sqrt(N(gx2)) = N(Z u^2) N(u) (N(Z) N(gx1))^((p+1)/4) = N(Z u^2) N(u) 5^((p+1)/4) s1,
// where s1 = N(gx1)^((p+1)/4) is the candidate already computed.  The root of gx (x1 or
// x2) then costs one more exponentiation.  The result equals RFC 9380's: the square root
// is unique up to sign and the sign is fixed by sgn0 below.
//
// The one inversion, 1/tv1 = conj(tv1) / N(tv1), is split out so that a batch of sets can
// share one field inversion for all its N(tv1) (Montgomery's trick, done by the caller):
// sswu_tv1(u) gives tv1, and map_to_curve_sswu_ni(u, ni) finishes with ni = 1/N(tv1)
// (ni = 0 when tv1 = 0, the exceptional case, as fp_inv(0) = 0 gives).
LSG_INL fp2_t sswu_tv1(const fp2_t& u) {
  fp2_t zu2 = fp2_mul(SSWU_Z, fp2_sqr(u));
  return fp2_add(fp2_sqr(zu2), zu2);
}
LSG_INL fp2_t fp2_inv_with_norm_inv(const fp2_t& a, const fp_t& ni) {
  return fp2_t(fp_mul(a.c0, ni), fp_neg(fp_mul(a.c1, ni)));
}
// Cut at the two powers (which the stage kernels of lsg_k_hash.hip run outside, one element
// per lane): stage a up to gx1 and gx2 -- the first power takes N(gx1) --, stage b from the
// candidate s1 to the chosen x, gx and the second power's operand c, stage c from t = c^((p-3)/4)
// to the point.  map_to_curve_sswu_ni is the three composed.
struct sswu_mid_t {
  fp2_t zu2, x1, x2, gx1, gx2;
};
LSG_BIGFN sswu_mid_t sswu_stage_a(fp2_t u, fp_t ni) {
  sswu_mid_t m;
  fp2_t u2 = fp2_sqr(u);
  m.zu2 = fp2_mul(SSWU_Z, u2);
  fp2_t tv1 = fp2_add(fp2_sqr(m.zu2), m.zu2);
  bool exc = fp2_is_zero(tv1);
  fp2_t x1 = fp2_mul(SSWU_MINUS_B_OVER_A, fp2_add(fp2_one(), fp2_inv_with_norm_inv(tv1, ni)));
  m.x1 = fp2_select(exc, SSWU_B_OVER_ZA, x1);
  m.gx1 = fp2_add(fp2_mul(fp2_add(fp2_sqr(m.x1), SSWU_A), m.x1), SSWU_B);
  m.x2 = fp2_mul(m.zu2, m.x1);
  m.gx2 = fp2_add(fp2_mul(fp2_add(fp2_sqr(m.x2), SSWU_A), m.x2), SSWU_B);
  return m;
}
// n = N(gx1), s1 = n^((p+1)/4); x, gx: the chosen candidate; returns c (fp2_sqrt_root_c)
LSG_BIGFN fp_t sswu_stage_b(fp2_t& x, fp2_t& gx, const sswu_mid_t& m, const fp2_t& u, const fp_t& n, const fp_t& s1) {
  bool sq1 = fp_is_root_of(s1, n);
  fp_t s2 = fp_mul(fp_mul(fp2_norm(m.zu2), fp2_norm(u)), fp_mul(s1, fp_t(SSWU_NZ_POW_P1D4)));
  x = fp2_select(sq1, m.x1, m.x2);
  gx = fp2_select(sq1, m.gx1, m.gx2);
  return fp2_sqrt_root_c(gx, fp_select(sq1, s1, s2));
}
LSG_BIGFN g2a_t sswu_stage_c(const fp2_t& u, const fp2_t& x, const fp2_t& gx, const fp_t& c, const fp_t& t) {
  g2a_t r;
  r.x = x;
  fp2_t y;
  (void)fp2_sqrt_root_finish(y, gx, c, t);
  if (fp2_sgn0(u) != fp2_sgn0(y)) y = fp2_neg(y);
  r.y = y;
  return r;
}
LSG_BIGFN g2a_t map_to_curve_sswu_ni(fp2_t u, fp_t ni) {
  const sswu_mid_t m = sswu_stage_a(u, ni);
  fp_t n = fp2_norm(m.gx1);
  fp_t s1 = fp_pow_id(n, LSG_POW_SQRT);
  fp2_t x, gx;
  fp_t c = sswu_stage_b(x, gx, m, u, n, s1);
  fp_t t = fp_pow_id(c, LSG_POW_SQRT34);
  return sswu_stage_c(u, x, gx, c, t);
}
LSG_BIGFN g2a_t map_to_curve_sswu(fp2_t u) { return map_to_curve_sswu_ni(u, fp_inv(fp2_norm(sswu_tv1(u)))); }

// 3-isogeny E2' -> E2, projective output (X, Y, Z) = (xn yd, y yn xd, xd yd)
LSG_BIGFN g2p_t iso_map3(g2a_t p) {
  const fp2_t& x = p.x;
  fp2_t xn = fp2_add(fp2_mul(fp2_add(fp2_mul(fp2_add(fp2_mul(ISO_XNUM_3, x), ISO_XNUM_2), x), ISO_XNUM_1), x),
                     ISO_XNUM_0);
  fp2_t xd = fp2_add(fp2_mul(fp2_add(x, ISO_XDEN_1), x), ISO_XDEN_0);
  fp2_t yn = fp2_add(fp2_mul(fp2_add(fp2_mul(fp2_add(fp2_mul(ISO_YNUM_3, x), ISO_YNUM_2), x), ISO_YNUM_1), x),
                     ISO_YNUM_0);
  fp2_t yd = fp2_add(fp2_mul(fp2_add(fp2_mul(fp2_add(x, ISO_YDEN_2), x), ISO_YDEN_1), x), ISO_YDEN_0);
  g2p_t r;
  r.X = fp2_mul(xn, yd);
  r.Y = fp2_mul(fp2_mul(p.y, yn), xd);
  r.Z = fp2_mul(xd, yd);
  if (fp2_is_zero(r.Z)) r = proj_inf<fp2_t>();
  return r;
}

// h_eff * P = [x^2 - x - 1]P + [x - 1]psi(P) + psi^2(2P)   (RFC 9380 appendix G.3), as
// c + [x]([x]P + psi(P)) with c = psi^2(2P) - psi(P) - P - [x]P: the terms are folded into c
// as soon as they exist, so each [x] chain runs with one other point live (registers, not
// scratch).
LSG_BIGFN g2p_t clear_cofactor_g2(g2p_t p) {
  const g2p_t u = g2_psi(p);
  g2p_t c = g2_add(g2_psi2(g2_dbl(p)), proj_neg(u));
  c = g2_add(c, proj_neg(p));
  const g2p_t t1 = proj_neg(proj_mul_xabs(p));  // [x]P
  c = g2_add(c, proj_neg(t1));
  const g2p_t t2 = proj_neg(proj_mul_xabs(g2_add(t1, u)));  // [x]([x]P + psi(P))
  return g2_add(c, t2);
}
// The same sum for a per-set kernel with one parked point (get/put: a per-lane LDS slot
// holding P on entry) and one point parked in the caller's global slot (cput/cget): the [x]
// chains run with their base in LDS and only the accumulator in registers, and no step in
// between holds more than two points.
// LANES: the two [x] chains run their doublings with one Fp2 component per lane
// (g2_mul_xabs_get_dbl_lanes, lsg_curve.hpp); the additions, the sums between the chains, psi
// and psi^2 are in the pair form either way.
template <bool LANES = false, class G, class P, class CP, class CG>
LSG_INL g2p_t clear_cofactor_g2_parked(const G& get, const P& put, const CP& cput, const CG& cget) {
  auto xabs = [&]() {
#ifdef LSG_FP2_LANES
    if (LANES) return g2_mul_xabs_get_dbl_lanes(get);
#endif
    return proj_mul_xabs_get<fp2_t>(get);
  };
  cput(proj_neg(xabs()));  // t1 = [x]P
  g2p_t c;
  {
    const g2p_t p = get();
    c = g2_add(g2_psi2(g2_dbl(p)), proj_neg(p));
    put(g2_psi(p));  // u = psi(P)
  }
  c = g2_add(c, proj_neg(get()));
  const g2p_t t1 = cget();
  cput(g2_add(c, proj_neg(t1)));  // c = psi^2(2P) - P - psi(P) - [x]P
  put(g2_add(t1, get()));         // [x]P + psi(P)
  const g2p_t t2 = proj_neg(xabs());  // [x]([x]P + psi(P))
  return g2_add(cget(), t2);
}
