// lsg_k_reduce.hip -- segmented reductions of lane-form values (G1/G2 sums, Fp12 products),
// batched field inversions, canonical-blob conversions and the roofline probes.
//
// The segmented reduction serves every "sum over a list" of the path with one launch per pass:
//   PublicKey.aggregate of each set's keys      (utils.ts:11)      G1 add
//   the RLC bucket MSM: buckets, per-bit sums   (blst mul_n_aggregate; 8a M4)      G2 add
//   small groups' signature sums, op-pool sums  (8a M4, 8f(4))                     G2 add
//   each group's Miller product                 (blst miller_loop_n/commit; 8a M5) Fp12 mul
// A chunk (a list of up to ips x F elements) belongs to 2^ips_log2 lane pairs of one wave:
// pair j folds elements j, j + ips, j + 2 ips, ... serially (every fold is a full-width
// SIMD operation), then the ips partial values are combined by a butterfly over lanes
// (shuffles, no LDS round trip).  Segments longer than one chunk get a second pass over the
// chunk results (lsg_plan.hpp plan_seg), so a reduction is one or two launches instead of
// one launch per tree level.
#include "lsg_kcommon.hpp"
namespace {
#include "lsg_inv.hpp"
}  // namespace

template <int OP>
struct seg_op;
template <>
struct seg_op<0> {
  typedef g1p_t T;
  static LSG_DEVI T ident() { return proj_inf<fp_t>(); }
  static LSG_DEVI T op(const T& a, const T& b) { return g1_add(a, b); }
};
template <>
struct seg_op<1> {
  typedef g2p_t T;
  static LSG_DEVI T ident() { return proj_inf<fp2_t>(); }
  static LSG_DEVI T op(const T& a, const T& b) { return g2_add(a, b); }
};
template <>
struct seg_op<2> {
  typedef fp12_t T;
  static LSG_DEVI T ident() { return fp12_one(); }
  static LSG_DEVI T op(const T& a, const T& b) { return fp12_mul(a, b); }
};

// Every lane runs the butterfly (no early return): a chunk's lanes are all active or all
// inactive, and a chunk never straddles a wave (ips <= 32 pairs, chunk-aligned items).
template <int OP>
__global__ void LSG_KERNEL_ATTR_W(OP == 2 ? 1 : LSG_WAVES_PER_EU)
    k_seg_reduce(int n_chunks, int ips_log2, const int32_t* __restrict__ chunks, const int32_t* __restrict__ idx,
                 const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t* __restrict__ tmp) {
  typedef seg_op<OP> O;
  typedef typename O::T T;
  lsg_lane_setup();
  const size_t item = gtid() / LSG_GROUP;
  const size_t c = item >> ips_log2;
  const int ips = 1 << ips_log2, j = (int)(item & (size_t)(ips - 1));
  const bool active = c < (size_t)n_chunks;
  T acc = O::ident();
  int out = 0;
  if (active) {
    const int off = chunks[3 * c], len = chunks[3 * c + 1];
    out = chunks[3 * c + 2];
    if (j < len) {
      acc = lane_load<T>(src, idx ? (size_t)idx[off + j] : (size_t)(off + j));
#pragma unroll 1
      for (int k = j + ips; k < len; k += ips) acc = O::op(acc, lane_load<T>(src, idx ? (size_t)idx[off + k] : (size_t)(off + k)));
    }
  }
#pragma unroll 1
  for (int o = ips >> 1; o >= 1; o >>= 1) acc = O::op(acc, shfl_xor_t(acc, LSG_GROUP * o));
  if (active && j == 0) {
    if (out >= 0)
      lane_store(dst, (size_t)out, acc);
    else
      lane_store(tmp, (size_t)(-out - 1), acc);
  }
}

// ---- batched field inversion (Montgomery's trick, chunked): every field inversion of a
// stage -- 1/Z of the scaled pubkeys, 1/N(tv1) of the SSWU maps, 1/N(Z) of the hashed points
// -- shares one exponentiation per batch instead of one per set.  A level folds chunks of
// LSG_BINV_T consecutive values per lane pair (prefix products, one chunk product each); the
// chunk products are the next level's values, up to one value, whose inverse unfolds back
// down (two products per value).  log_T(n) launches each way instead of log_2(n).  Zero
// inputs (points at infinity, the SSWU exceptional case) are carried as 1 and come out as 0,
// the value fp_inv(0) gives.
__global__ void LSG_KERNEL_ATTR k_binv_fold(int n, int zero_to_one, const uint32_t* __restrict__ in,
                                            uint32_t* __restrict__ pre, uint32_t* __restrict__ tot) {
  const int n_chunks = (n + LSG_BINV_T - 1) / LSG_BINV_T;
  LANE_ITEM(n_chunks);
  (void)lead;
  const fp_t one = fp_one();
  const int first = (int)item * LSG_BINV_T, last = min(n, first + LSG_BINV_T);
  fp_t acc = one;
#pragma unroll 1
  for (int k = first; k < last; k++) {
    fp_t x = lane_load<fp_t>(in, k);
    if (zero_to_one) x = fp_select(fp_is_zero(x), one, x);
    acc = k == first ? x : fp_mul(acc, x);
    lane_store(pre, k, acc);
  }
  lane_store(tot, item, acc);
}
// the one inversion of a batched inversion: the divstep GCD (lsg_inv.hpp, ~30 us) instead of
// the ~455-product Fermat chain (~0.4 ms of dependent products on one lane pair)
__global__ void LSG_KERNEL_ATTR k_binv_root(const uint32_t* __restrict__ top, uint32_t* __restrict__ inv) {
  LANE_ITEM(1);
  (void)lead;
  const fp_t d = pair_inv_gcd(pair_canon(lane_load<fp_t>(top, 0)));  // (x R)^-1 as an integer, 0 -> 0
  lane_store(inv, 0, pair_mont_mul(d, fp_t(FP_RCUBE)));              // x^-1 R
}
// out[k] = 1 / in[k] from the chunk's inverse product tinv[chunk] and the prefix products
__global__ void LSG_KERNEL_ATTR k_binv_unfold(int n, int zero_to_one, const uint32_t* __restrict__ in,
                                              const uint32_t* __restrict__ pre, const uint32_t* __restrict__ tinv,
                                              uint32_t* __restrict__ out) {
  const int n_chunks = (n + LSG_BINV_T - 1) / LSG_BINV_T;
  LANE_ITEM(n_chunks);
  (void)lead;
  const fp_t one = fp_one();
  const int first = (int)item * LSG_BINV_T, last = min(n, first + LSG_BINV_T);
  fp_t acc = lane_load<fp_t>(tinv, item);  // 1 / (in[first] * ... * in[last-1])
#pragma unroll 1
  for (int k = last - 1; k >= first; k--) {
    fp_t x = lane_load<fp_t>(in, k);
    const bool z = zero_to_one && fp_is_zero(x);
    fp_t r = k > first ? fp_mul(acc, lane_load<fp_t>(pre, k - 1)) : acc;
    lane_store(out, k, z ? fp_zero() : r);
    if (k > first && !z) acc = fp_mul(acc, x);
  }
}

// One-launch batched inversion: every workgroup inverts its own share --
// lane pair l of block b folds the T consecutive values from (b * 128 + l) * T into prefix
// products, the block's 128 chunk products go through an LDS heap with ONE divstep inversion
// at its root (block_inv), and each lane pair unfolds its chunk.  No level crosses a block,
// so the fold / root / unfold launches of the multi-level form (2 log16 n + 1 of them, each a
// latency-bound stub between real kernels) become one.  zero_to_one: zeros fold as one and
// come out as zero (fp_inv(0) = 0).
__global__ void LSG_KERNEL_ATTR k_binv_block(int n, int T, int zero_to_one, const uint32_t* __restrict__ in,
                                             uint32_t* __restrict__ pre, uint32_t* __restrict__ out) {
  __shared__ uint32_t H[2 * LSG_ITEMS_PER_BLOCK * lsgl::W_FP], I[2 * LSG_ITEMS_PER_BLOCK * lsgl::W_FP];
  lsg_lane_setup();
  const int l = (int)(threadIdx.x / LSG_GROUP);
  const int64_t first = ((int64_t)blockIdx.x * LSG_ITEMS_PER_BLOCK + l) * T;
  const int64_t last = first + T < (int64_t)n ? first + T : (int64_t)n;
  const fp_t one = fp_one();
  fp_t acc = one;
#pragma unroll 1
  for (int64_t k = first; k < last; k++) {
    fp_t x = lane_load<fp_t>(in, (size_t)k);
    if (zero_to_one) x = fp_select(fp_is_zero(x), one, x);
    acc = k == first ? x : fp_mul(acc, x);
    if (T > 1) lane_store(pre, (size_t)k, acc);
  }
  fp_t inv = block_inv<LSG_ITEMS_PER_BLOCK>(H, I, l, acc);  // every lane pair is a leaf (one when idle)
#pragma unroll 1
  for (int64_t k = last - 1; k >= first; k--) {
    const fp_t x = lane_load<fp_t>(in, (size_t)k);
    const bool z = zero_to_one && fp_is_zero(x);
    const fp_t r = k > first ? fp_mul(inv, lane_load<fp_t>(pre, (size_t)k - 1)) : inv;
    lane_store(out, (size_t)k, z ? fp_zero() : r);
    if (k > first && !z) inv = fp_mul(inv, x);
  }
}

// partials: canonical big-endian 576-byte Fp12 blobs <-> lane form (one item each)
__global__ void LSG_KERNEL_ATTR k_blobs_to_fp12(int n, const uint8_t* __restrict__ blobs, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  lane_store(out, item, fp12_from_canon_bytes(blobs + 576 * item));
}
__global__ void LSG_KERNEL_ATTR k_fp12_to_canon(int n, const uint32_t* __restrict__ in, uint8_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  fp12_to_canon_bytes(out + 576 * item, lane_load<fp12_t>(in, item));
}

// f^r for a nonzero 64-bit r (square-and-multiply, one item): the partial of a package group
// that is one set verified unscaled leaves the slot as f^r, so that FE(product of partials) is
// the RLC check prod_i e_i^(r_i) whatever the other partials are (FE(f^r) = FE(f)^r)
__global__ void LSG_KERNEL_ATTR_W(1) k_fp12_pow_u64(const uint8_t* __restrict__ in576, uint64_t r,
                                                    uint8_t* __restrict__ out576) {
  LANE_ITEM(1);
  (void)lead;
  const fp12_t f = fp12_from_canon_bytes(in576);
  fp12_t acc = f;
  int top = 63;
  while (top > 0 && !((r >> top) & 1u)) top--;
#pragma unroll 1
  for (int b = top - 1; b >= 0; b--) {
    // (the sums carried one operation at a time: as lazy sums this kernel's scratch grew, 784 -> 1056 B)
    acc = fp12_sqr<false>(acc);
    if ((r >> b) & 1u) acc = fp12_mul<false>(acc, f);
  }
  fp12_to_canon_bytes(out576, acc);
}

// parity hook of the Fp2 product leaf (pair_fp2_mul_v: the SOP form) at its lazy bounds: per
// item, c0 + c1 u = (a0 + a1 u)(b0 + b1 u) R^-1 from four raw pair-layout operands, stored raw
// (not reduced, not canonical) so that the test checks the value and the leaf's output bound
__global__ void LSG_KERNEL_ATTR k_check_fp2_mul(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  const fp2_t a(lane_load<fp_t>(in, 4 * item), lane_load<fp_t>(in, 4 * item + 1));
  const fp2_t b(lane_load<fp_t>(in, 4 * item + 2), lane_load<fp_t>(in, 4 * item + 3));
  const fp2_t c = fp2_mul(a, b);
  lane_store(out, 2 * item, c.c0);
  lane_store(out, 2 * item + 1, c.c1);
}
// the same hooks for the squaring leaves (fp_sqr: pair_mont_sqr, fp2_sqr: pair_fp2_sqr_v)
__global__ void LSG_KERNEL_ATTR k_check_fp_sqr(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  lane_store(out, item, fp_sqr(lane_load<fp_t>(in, item)));
}
__global__ void LSG_KERNEL_ATTR k_check_fp2_sqr(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  const fp2_t c = fp2_sqr(fp2_t(lane_load<fp_t>(in, 2 * item), lane_load<fp_t>(in, 2 * item + 1)));
  lane_store(out, 2 * item, c.c0);
  lane_store(out, 2 * item + 1, c.c1);
}
// parity hook of the lazy sums (lsg_fp_pair.hpp fps_t, lsg_tower.hpp fp2s_t) at the lazy bounds.
// The 12 n raw input elements form a ring; item i works on el(j) = element 12 i + j.  Per item
// LSG_CHECK_SUMS_OUT elements, stored raw:
//    0      (a + b + c - d - e - f).carry(), the maximal admissible chain
//    1..5   2a, 3a, 4a, 8a, 12a (carry_mul)
//    6..7   fp2_mul_b3(a + b u)
//    8..10  jac_dbl over Fp of (a, b, c);          11..13  the same one carried operation at a time
//   14..19  jac_dbl over Fp2 of (el 0..5);         20..25  the same one carried operation at a time
//   26..31  proj_add over Fp2 of (el 0..5), (el 6..11);  32..37  the same one operation at a time
//   38..39  mfc_mul<3> on V(p) = (el 2p, el 2p + 1), the fused Miller kernel's longest combination;
//   40..41  its nested form
template <class F>
LSG_DEVI jac_t<F> check_jac_dbl_nested(const jac_t<F>& p) {
  F A = fsqr(p.X), B = fsqr(p.Y), C = fsqr(B);
  F D = fsub(fsqr(fadd(p.X, B)), fadd(A, C));
  D = fadd(D, D);
  F E = fadd(fadd(A, A), A);
  F Fq = fsqr(E);
  jac_t<F> r;
  r.X = fsub(Fq, fadd(D, D));
  F C8 = fadd(C, C);
  C8 = fadd(C8, C8);
  C8 = fadd(C8, C8);
  r.Y = fsub(fmul(E, fsub(D, r.X)), C8);
  F yz = fmul(p.Y, p.Z);
  r.Z = fadd(yz, yz);
  return r;
}
LSG_DEVI fp2_t check_b3_nested(const fp2_t& a) {
  auto m12 = [](const fp_t& x) {
    const fp_t x4 = fp_dbl(fp_dbl(x));
    return fp_add(fp_dbl(x4), x4);
  };
  return fp2_t(m12(fp_sub(a.c0, a.c1)), m12(fp_add(a.c0, a.c1)));
}
LSG_DEVI g2p_t check_proj_add_nested(const g2p_t& p, const g2p_t& q) {
  typedef fp2_t F;
  F t0 = fmul(p.X, q.X), t1 = fmul(p.Y, q.Y), t2 = fmul(p.Z, q.Z);
  F t3 = fmul(fadd(p.X, p.Y), fadd(q.X, q.Y));
  F t4 = fadd(t0, t1);
  t3 = fsub(t3, t4);
  t4 = fmul(fadd(p.Y, p.Z), fadd(q.Y, q.Z));
  F X3 = fadd(t1, t2);
  t4 = fsub(t4, X3);
  X3 = fmul(fadd(p.X, p.Z), fadd(q.X, q.Z));
  F Y3 = fadd(t0, t2);
  Y3 = fsub(X3, Y3);
  X3 = fadd(t0, t0);
  t0 = fadd(X3, t0);
  t2 = check_b3_nested(t2);
  F Z3 = fadd(t1, t2);
  t1 = fsub(t1, t2);
  Y3 = check_b3_nested(Y3);
  X3 = fmul(t4, Y3);
  t2 = fmul(t3, t1);
  X3 = fsub(t2, X3);
  Y3 = fmul(Y3, t0);
  t1 = fmul(t1, Z3);
  Y3 = fadd(t1, Y3);
  t0 = fmul(t0, t3);
  Z3 = fmul(Z3, t4);
  Z3 = fadd(Z3, t0);
  return g2p_t{X3, Y3, Z3};
}
constexpr int LSG_CHECK_SUMS_IN = 12, LSG_CHECK_SUMS_OUT = 42;
__global__ void LSG_KERNEL_ATTR k_check_sums(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  const size_t ring = (size_t)LSG_CHECK_SUMS_IN * (size_t)n;
  auto el = [&](int j) { return lane_load<fp_t>(in, ((size_t)LSG_CHECK_SUMS_IN * item + (size_t)j) % ring); };
  auto el2 = [&](int j) { return fp2_t(el(2 * j), el(2 * j + 1)); };
  int o = 0;
  auto put = [&](const fp_t& v) { lane_store(out, (size_t)LSG_CHECK_SUMS_OUT * item + (size_t)(o++), v); };
  auto put2 = [&](const fp2_t& v) {
    put(v.c0);
    put(v.c1);
  };
  const fp_t a = el(0), b = el(1), c = el(2);
  put((fps(a) + b + c - el(3) - el(4) - el(5)).carry());
  put(fp_mulk<2>(a));
  put(fp_mulk<3>(a));
  put(fp_mulk<4>(a));
  put(fp_mulk<8>(a));
  put(fp_mulk<12>(a));
  put2(fp2_mul_b3(fp2_t(a, b)));
  const jac_t<fp_t> j1 = {a, b, c};
  const jac_t<fp_t> r1 = jac_dbl(j1), n1 = check_jac_dbl_nested(j1);
  put(r1.X), put(r1.Y), put(r1.Z);
  put(n1.X), put(n1.Y), put(n1.Z);
  const jac_t<fp2_t> j2 = {el2(0), el2(1), el2(2)};
  const jac_t<fp2_t> r2 = jac_dbl(j2), n2 = check_jac_dbl_nested(j2);
  put2(r2.X), put2(r2.Y), put2(r2.Z);
  put2(n2.X), put2(n2.Y), put2(n2.Z);
  const g2p_t p = {el2(0), el2(1), el2(2)}, q = {el2(3), el2(4), el2(5)};
  const g2p_t r3 = g2_add(p, q), n3 = check_proj_add_nested(p, q);
  put2(r3.X), put2(r3.Y), put2(r3.Z);
  put2(n3.X), put2(n3.Y), put2(n3.Z);
  // t2_0 - t0_0 - xi n2 of the M phase (lsg_k_miller.hip mf_mul_pair, lsg_pairing.hpp mfc_mul)
  put2(mfc_mul<3>(el2));
  const fp2_t t2c = fp2_add(el2(11), fp2_mul_xi(fp2_sub(fp2_sub(el2(15), el2(12)), el2(13))));
  const fp2_t t0c = fp2_add(el2(0), fp2_mul_xi(fp2_sub(fp2_sub(el2(4), el2(1)), el2(2))));
  put2(fp2_sub(fp2_sub(t2c, t0c), fp2_mul_xi(fp2_add(el2(7), el2(9)))));
}

// parity hooks of the component-per-lane Fp2 layout (lsg_fp2_lanes.hpp) on caller-chosen limbs.
// k_check_fp2_lanes: 12 raw pair-layout elements per item in = the Fp2 values A..F
// (X = (el 2j, el 2j + 1)); 12 Fp2 values per item out, raw, every one but the last converted
// back to the pair layout:
//    0  A through the conversion in and out      1  A B      2  A^2
//    3  (A + B + C - D - E - F).carry()          4..8  2A, 3A, 4A, 8A, 12A (carry_mul)
//    9  fmul_b3(A)                               10  -A
//   11  A in the lane layout as the lanes hold it: word k of lane h at 2 k + h (pins which
//       lane holds which component)
// k_check_g2_lanes: 12 elements in = a Jacobian point J = (A, B, C) and a homogeneous point
// Q = (D, E, F); out: jac_dbl(J) in the lane layout, in the pair layout, jac_add_proj(J, Q) in the
// lane layout, in the pair layout (3 Fp2 values each).
#ifdef LSG_FP2_LANES
__global__ void LSG_KERNEL_ATTR k_check_fp2_lanes(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  auto el2 = [&](int j) {
    return fp2_t(lane_load<fp_t>(in, (size_t)lsgk::CHECK_LANES_IN * item + 2 * j),
                 lane_load<fp_t>(in, (size_t)lsgk::CHECK_LANES_IN * item + 2 * j + 1));
  };
  int o = 0;
  auto put = [&](const fp2v_t& v) {
    const fp2_t w = fp2v_to_pair(v);
    lane_store(out, (size_t)lsgk::CHECK_LANES_OUT * item + (size_t)o, w.c0);
    lane_store(out, (size_t)lsgk::CHECK_LANES_OUT * item + (size_t)o + 1, w.c1);
    o += 2;
  };
  const fp2v_t A = fp2v_from_pair(el2(0)), B = fp2v_from_pair(el2(1)), C = fp2v_from_pair(el2(2));
  const fp2v_t D = fp2v_from_pair(el2(3)), E = fp2v_from_pair(el2(4)), F = fp2v_from_pair(el2(5));
  put(A);
  put(fmul(A, B));
  put(fsqr(A));
  put((fsum(A) + B + C - D - E - F).carry());
  put(fmulk<2>(A));
  put(fmulk<3>(A));
  put(fmulk<4>(A));
  put(fmulk<8>(A));
  put(fmulk<12>(A));
  put(fmul_b3(A));
  put(fneg(A));
  lane_store(out + (size_t)lsgk::CHECK_LANES_OUT * lsgl::W_FP * item + (size_t)o * lsgl::W_FP, 0, A);
}
__global__ void LSG_KERNEL_ATTR k_check_g2_lanes(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  auto el2 = [&](int j) {
    return fp2_t(lane_load<fp_t>(in, (size_t)lsgk::CHECK_G2L_IN * item + 2 * j),
                 lane_load<fp_t>(in, (size_t)lsgk::CHECK_G2L_IN * item + 2 * j + 1));
  };
  int o = 0;
  auto put2 = [&](const fp2_t& w) {
    lane_store(out, (size_t)lsgk::CHECK_G2L_OUT * item + (size_t)o, w.c0);
    lane_store(out, (size_t)lsgk::CHECK_G2L_OUT * item + (size_t)o + 1, w.c1);
    o += 2;
  };
  auto putv = [&](const jac_t<fp2v_t>& r) { put2(fp2v_to_pair(r.X)), put2(fp2v_to_pair(r.Y)), put2(fp2v_to_pair(r.Z)); };
  auto putp = [&](const jac_t<fp2_t>& r) { put2(r.X), put2(r.Y), put2(r.Z); };
  const jac_t<fp2_t> J = {el2(0), el2(1), el2(2)};
  const g2p_t Q = {el2(3), el2(4), el2(5)};
  const jac_t<fp2v_t> Jv = {fp2v_from_pair(J.X), fp2v_from_pair(J.Y), fp2v_from_pair(J.Z)};
  putv(jac_dbl(Jv));
  putp(jac_dbl(J));
  putv(jac_add_proj(Jv, g2v_from_pair(Q)));
  putp(jac_add_proj(J, Q));
}
// k_check_mf_lanes: the pieces the fused Miller kernel adds to the layout; 12 elements in
// (A .. F as above), 24 out, each lane-layout result converted back beside its pair-form twin:
//    0  fmul_fp(A, B.c0)            1  fp2_mul_fp(A, B.c0)
//    2  fmul_xi(A)                  3  fp2_mul_xi(A)
//    4  A + xi (B - C), one carry   5  the same on fp2s_t
//    6..8  fp6_mul_v((A, B, C))     9  fone     10  fzero
//   11  B.c0 spread over both lanes (fpv_from_pair) as the lanes hold it: word k of lane h at 2 k + h
__global__ void LSG_KERNEL_ATTR k_check_mf_lanes(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  auto el2 = [&](int j) {
    return fp2_t(lane_load<fp_t>(in, (size_t)lsgk::CHECK_LANES_IN * item + 2 * j),
                 lane_load<fp_t>(in, (size_t)lsgk::CHECK_LANES_IN * item + 2 * j + 1));
  };
  int o = 0;
  auto put2 = [&](const fp2_t& w) {
    lane_store(out, (size_t)lsgk::CHECK_LANES_OUT * item + (size_t)o, w.c0);
    lane_store(out, (size_t)lsgk::CHECK_LANES_OUT * item + (size_t)o + 1, w.c1);
    o += 2;
  };
  auto put = [&](const fp2v_t& v) { put2(fp2v_to_pair(v)); };
  const fp2_t Ap = el2(0), Bp = el2(1), Cp = el2(2);
  const fp2v_t A = fp2v_from_pair(Ap), B = fp2v_from_pair(Bp), C = fp2v_from_pair(Cp);
  const fpv_t k = fpv_from_pair(Bp.c0);
  put(fmul_fp(A, k));
  put2(fp2_mul_fp(Ap, Bp.c0));
  put(fmul_xi(A));
  put2(fp2_mul_xi(Ap));
  put((fsum(A) + fsum_mul_xi(fsum(B) - C)).carry());
  put2((fp2s(Ap) + fp2s_mul_xi(fp2s(Bp) - Cp)).carry());
  const fp6v_t v = fp6_mul_v(fp6_make(A, B, C));
  put(v.c0);
  put(v.c1);
  put(v.c2);
  put(fone<fp2v_t>());
  put(fzero<fp2v_t>());
  lane_store(out + (size_t)lsgk::CHECK_LANES_OUT * lsgl::W_FP * item + (size_t)o * lsgl::W_FP, 0, k);
}
#endif

// parity hooks of the layer between the products and the accept / reject rules: canonical
// forms, the predicates on them, the byte conversions, the Fp2 root and the two inversions,
// on caller-chosen raw limbs.  Every output comes from the function the kernels call.
// k_check_canon: one raw element per item in, LSG_CHECK_CANON_OUT words per item out:
//    0..13  pair_canon(a)      14..27  fp_canonical(a)     28..39  fp_to_be48(fp_canonical(a))
//   40      bit 0 fp_is_zero(a), 1 fp_canon_lt_p(a), 2 fp_canon_gt_half(a), 3 fp_canon_parity(a)
//   41      0           42..53  fp_to_be48(a): the raw value's bytes (a in [0, 2^384), flag bits kept)
constexpr int LSG_CHECK_CANON_OUT = lsgk::CHECK_CANON_OUT;
__global__ void LSG_KERNEL_ATTR k_check_canon(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  const fp_t a = lane_load<fp_t>(in, item);
  uint32_t* o = out + (size_t)LSG_CHECK_CANON_OUT * item;
  const fp_t c = fp_canonical(a);
  lane_store(o, 0, pair_canon(a));
  lane_store(o + 14, 0, c);
  fp_to_be48((uint8_t*)(o + 28), c);
  fp_to_be48((uint8_t*)(o + 42), a);
  const uint32_t f = (fp_is_zero(a) ? 1u : 0u) | (fp_canon_lt_p(a) ? 2u : 0u) | (fp_canon_gt_half(a) ? 4u : 0u) |
                     (fp_canon_parity(a) ? 8u : 0u);
  o[40 + (lead ? 0 : 1)] = lead ? f : 0u;
}
// k_check_from_bytes: 48 big-endian bytes per item in, fp_from_be_bytes(b, 12) out (14 words)
__global__ void LSG_KERNEL_ATTR k_check_from_bytes(int n, const uint8_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  lane_store(out, item, fp_from_be_bytes(in + 48 * item, 12));
}
// k_check_fp2_roots: (a0, a1) in Montgomery form (lazy limbs allowed) per item in,
// LSG_CHECK_ROOTS_OUT words per item out:
//    0..27  the root fp2_sqrt leaves (c0, c1), raw      28..41  fp_inv(a0), raw
//   42..55  pair_mont_mul(pair_inv_gcd(pair_canon(a0)), FP_RCUBE), raw (k_binv_root, block_inv)
//   56      bit 0 fp2_sqrt's result, 1 fp2_sgn0(a), 2 fp2_lexi_largest(a), 3 fp2_is_zero(a)
//   57      0
constexpr int LSG_CHECK_ROOTS_OUT = lsgk::CHECK_ROOTS_OUT;
__global__ void LSG_KERNEL_ATTR k_check_fp2_roots(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  const fp2_t a(lane_load<fp_t>(in, 2 * item), lane_load<fp_t>(in, 2 * item + 1));
  uint32_t* o = out + (size_t)LSG_CHECK_ROOTS_OUT * item;
  fp2_t r;
  const bool ok = fp2_sqrt(r, a);
  lane_store(o, 0, r.c0);
  lane_store(o + 14, 0, r.c1);
  lane_store(o + 28, 0, fp_inv(a.c0));
  lane_store(o + 42, 0, pair_mont_mul(pair_inv_gcd(pair_canon(a.c0)), fp_t(FP_RCUBE)));
  const uint32_t f = (ok ? 1u : 0u) | (fp2_sgn0(a) ? 2u : 0u) | (fp2_lexi_largest(a) ? 4u : 0u) |
                     (fp2_is_zero(a) ? 8u : 0u);
  o[56 + (lead ? 0 : 1)] = lead ? f : 0u;
}

// The fixed-exponent powers of the signature decompression and the SSWU map (lsg_k_sig.hip,
// lsg_k_hash.hip: the stage kernels around them) with one Fp element per lane
// (lsg_fp2_lanes.hpp fpl_t): out[i] = in[i]^e for the plan LSG_POW_PLANS[id], word for word
// pair_pow_plan's.  in / out: fp_t arrays in the pair item-major layout (lane_store<fp_t>).  No
// LDS, no barrier, no cross-lane step; lanes beyond n leave at once.
#ifndef LSG_POW_LANES_WAVES
#define LSG_POW_LANES_WAVES 2
#endif
__global__ void LSG_KERNEL_ATTR_W(LSG_POW_LANES_WAVES) k_fp_pow_lanes(int n, int id, const uint32_t* __restrict__ in,
                                                                      uint32_t* __restrict__ out) {
  const size_t i = gtid();
  if (i >= (size_t)n) return;
  id = __builtin_amdgcn_readfirstlane(id);
  lanes_fp_store(out, i, lanes_pow_plan(lanes_fp_load(in, i), id));
}
// k_check_pow_pair: the pair form's pair_pow_plan on the same arrays (the device tests' reference)
__global__ void LSG_KERNEL_ATTR k_check_pow_pair(int n, int id, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  lane_store(out, item, fp_pow_id(lane_load<fp_t>(in, item), id));
}

// roofline probe: 4 independent limb-parallel Montgomery chains per pair
__global__ void LSG_KERNEL_ATTR k_probe_fp_mul(int n, int iters, uint32_t* __restrict__ io) {
  LANE_ITEM(n);
  (void)lead;
  fp_t a = lane_load<fp_t>(io, item), b = fp_t(FP_R2), c = fp_t(FP_R3), d = fp_t(FP_HALF);
  for (int k = 0; k < iters; k++) {
    a = fp_mul(a, b);
    b = fp_mul(b, c);
    c = fp_mul(c, d);
    d = fp_mul(d, a);
  }
  lane_store(io, item, fp_add(fp_add(a, b), fp_add(c, d)));
}

// roofline probe: raw v_mad_u64_u32 issue rate, 16 independent 64-bit accumulators per lane
__global__ void __launch_bounds__(256) k_probe_mad(int iters, uint32_t seed, uint64_t* __restrict__ io) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t acc[16];
  uint32_t x[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    acc[k] = t + k;
    x[k] = (t * 2654435761u) ^ (seed + 977u * k);
  }
  const uint32_t y = seed | 1u;
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = (uint64_t)x[k] * y + acc[k];
  }
  uint64_t r = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) r ^= acc[k];
  io[t] = r;
}

namespace lsgk {
hipError_t seg_reduce(hipStream_t st, int op, int n_chunks, int ips_log2, const int32_t* chunks, const int32_t* idx,
                      const uint32_t* src, uint32_t* dst, uint32_t* tmp) {
  const size_t items = (size_t)n_chunks << ips_log2;
  if (op == 0) LSG_LAUNCH_ITEMS(k_seg_reduce<0>, items, st, n_chunks, ips_log2, chunks, idx, src, dst, tmp);
  if (op == 1) LSG_LAUNCH_ITEMS(k_seg_reduce<1>, items, st, n_chunks, ips_log2, chunks, idx, src, dst, tmp);
  LSG_LAUNCH_ITEMS(k_seg_reduce<2>, items, st, n_chunks, ips_log2, chunks, idx, src, dst, tmp);
}
hipError_t binv_fold(hipStream_t st, int n, int zero_to_one, const uint32_t* in, uint32_t* pre, uint32_t* tot) {
  LSG_LAUNCH_ITEMS(k_binv_fold, (n + LSG_BINV_T - 1) / LSG_BINV_T, st, n, zero_to_one, in, pre, tot);
}
hipError_t binv_block(hipStream_t st, int n, int T, int zero_to_one, const uint32_t* in, uint32_t* pre, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  const size_t chunks = ((size_t)n + T - 1) / T;
  hipLaunchKernelGGL(k_binv_block, dim3(lane_blocks(chunks)), dim3(LSG_TPB), 0, st, n, T, zero_to_one, in, pre, out);
  return hipGetLastError();
}
hipError_t binv_root(hipStream_t st, const uint32_t* top, uint32_t* inv) {
  LSG_LAUNCH_ITEMS(k_binv_root, 1, st, top, inv);
}
hipError_t binv_unfold(hipStream_t st, int n, int zero_to_one, const uint32_t* in, const uint32_t* pre,
                       const uint32_t* tinv, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_binv_unfold, (n + LSG_BINV_T - 1) / LSG_BINV_T, st, n, zero_to_one, in, pre, tinv, out);
}
hipError_t blobs_to_fp12(hipStream_t st, int n, const uint8_t* blobs, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_blobs_to_fp12, n, st, n, blobs, out);
}
hipError_t fp12_to_canon(hipStream_t st, int n, const uint32_t* in, uint8_t* out576) {
  LSG_LAUNCH_ITEMS(k_fp12_to_canon, n, st, n, in, out576);
}
hipError_t fp12_pow_u64(hipStream_t st, const uint8_t* in576, uint64_t r, uint8_t* out576) {
  LSG_LAUNCH_ITEMS(k_fp12_pow_u64, 1, st, in576, r, out576);
}
hipError_t check_fp2_mul(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_fp2_mul, n, st, n, in, out);
}
hipError_t check_fp_sqr(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_fp_sqr, n, st, n, in, out);
}
hipError_t check_fp2_sqr(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_fp2_sqr, n, st, n, in, out);
}
hipError_t check_sums(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_sums, n, st, n, in, out);
}
#ifdef LSG_FP2_LANES
hipError_t check_fp2_lanes(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_fp2_lanes, n, st, n, in, out);
}
hipError_t check_g2_lanes(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_g2_lanes, n, st, n, in, out);
}
hipError_t check_mf_lanes(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_mf_lanes, n, st, n, in, out);
}
#endif
hipError_t check_canon(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_canon, n, st, n, in, out);
}
hipError_t check_from_bytes(hipStream_t st, int n, const uint8_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_from_bytes, n, st, n, in, out);
}
hipError_t check_fp2_roots(hipStream_t st, int n, const uint32_t* in, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_check_fp2_roots, n, st, n, in, out);
}
hipError_t fp_pow_lanes(hipStream_t st, int n, int id, const uint32_t* in, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  if (id < 0 || id > 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fp_pow_lanes, dim3((unsigned)(((size_t)n + LSG_TPB - 1) / LSG_TPB)), dim3(LSG_TPB), 0, st, n, id,
                     in, out);
  return hipGetLastError();
}
hipError_t check_pow_pair(hipStream_t st, int n, int id, const uint32_t* in, uint32_t* out) {
  if (id < 0 || id > 2) return hipErrorInvalidValue;
  LSG_LAUNCH_ITEMS(k_check_pow_pair, n, st, n, id, in, out);
}
hipError_t probe_fp_mul(hipStream_t st, int items, int iters, uint32_t* io) {
  LSG_LAUNCH_ITEMS(k_probe_fp_mul, items, st, items, iters, io);
}
hipError_t probe_mad(hipStream_t st, int blocks, int iters, uint32_t seed, uint64_t* io) {
  if (blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_probe_mad, dim3(blocks), dim3(256), 0, st, iters, seed, io);
  return hipGetLastError();
}
}  // namespace lsgk
