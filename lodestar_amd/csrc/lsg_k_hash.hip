// lsg_k_hash.hip -- hash_to_G2 kernels (RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_ with the POP
// DST, blst's Hash_to_G2 inside Pairing.mul_n_aggregate under
// packages/beacon-node/src/chain/bls/maybeBatch.ts:18,37) and the SSZ
// signing roots of SURVEY.md 8f(3) (util/signingRoot.ts:7-13).
//
//   k_expand_msg   expand_message_xmd(msg_i, DST, 256), one thread per set (SHA-256)
//   k_h2c_prep     hash_to_field -> u0, u1; norms N(tv1(u0)), N(tv1(u1)) for one batched inversion
//   k_h2c_map      SSWU (shared-norm square root) -> 3-isogeny, one per field element; Q0 + Q1
//   k_h2c_clear    clear_cofactor (psi form); N(Z) for the second batched inversion
//   k_h2c_affine   (X, Y) * conj(Z) / N(Z)
//   k_h2c_cache_merge / k_h2c_cache_store   points read from / copied into the message cache
#include "lsg_kcommon.hpp"

// waves per SIMD for the SSWU map and the cofactor clearing: 2 (256 registers, some scratch)
// or 1 (512 registers, none)
#ifndef LSG_H2C_WAVES
#define LSG_H2C_WAVES 2
#endif

// expand_message_xmd(msg_i, DST, 256) (RFC 9380 5.3.1; oracle/hash_to_curve.py), one thread
// per message.  Each thread's SHA-256 block buffer lives in LDS, byte k of thread t at word
// (k / 4) * 64 + t (consecutive threads, consecutive banks): a byte appended is one LDS byte
// store, where a register array indexed by the byte count went to scratch (a read-modify-
// write per byte).  The Z_pad block is compressed without being written; b_i's 32-byte prefix
// is stored as words; the output goes to global memory as words.
struct ShaLds {
  uint32_t st[8];
  uint32_t n, total;
  uint8_t* blk;  // this thread's byte 0; byte k at blk[(k >> 2) * 256 + (k & 3)]
};
LSG_DEVI void shal_init(ShaLds& c) {
  const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
  for (int i = 0; i < 8; i++) c.st[i] = iv[i];
  c.n = 0;
  c.total = 0;
}
LSG_DEVI void shal_flush(ShaLds& c) {
  uint32_t w[16];
  const uint32_t* wl = (const uint32_t*)c.blk;
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = __builtin_bswap32(wl[k * 64]);
  sha256_compress(c.st, w);
  c.n = 0;
}
LSG_DEVI void shal_byte(ShaLds& c, uint8_t v) {
  c.blk[(c.n >> 2) * 256 + (c.n & 3)] = v;
  c.n++;
  c.total++;
  if (c.n == 64) shal_flush(c);
}
// a big-endian word at a word-aligned position (c.n % 4 == 0)
LSG_DEVI void shal_word(ShaLds& c, uint32_t v) {
  ((uint32_t*)c.blk)[(c.n >> 2) * 64] = __builtin_bswap32(v);
  c.n += 4;
  c.total += 4;
  if (c.n == 64) shal_flush(c);
}
LSG_DEVI void shal_final(ShaLds& c, uint32_t* out8) {
  const uint32_t bits = c.total * 8;  // (messages < 2^29 bytes)
  shal_byte(c, 0x80);
  while (c.n & 3) shal_byte(c, 0);
  if (c.n > 56)
    while (c.n) shal_word(c, 0);
  while (c.n < 60) shal_word(c, 0);
  shal_word(c, bits);
#pragma unroll
  for (int i = 0; i < 8; i++) out8[i] = c.st[i];
}

// append len bytes from src (global memory or LDS): the loads of 16 bytes are issued before
// the first append, so a lone message pays one memory round trip per 16 bytes, not per byte
LSG_DEVI void shal_bytes(ShaLds& c, const uint8_t* src, uint32_t len) {
  uint32_t k = 0;
  for (; k + 16 <= len; k += 16) {
    uint8_t b[16];
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = src[k + j];
#pragma unroll
    for (int j = 0; j < 16; j++) shal_byte(c, b[j]);
  }
  for (; k < len; k++) shal_byte(c, src[k]);
}

__global__ void __launch_bounds__(64) k_expand_msg(int n, const uint8_t* __restrict__ msg,
                                                    const uint32_t* __restrict__ msg_off,
                                                    const uint32_t* __restrict__ msg_len,
                                                    const uint8_t* __restrict__ dst, uint32_t dst_len,
                                                    uint8_t* __restrict__ ub) {
  __shared__ uint32_t lds[16 * 64];
  __shared__ uint8_t s_dst[256];  // the DST (< 256 bytes, RFC 9380), appended nine times
  for (uint32_t k = threadIdx.x; k < dst_len; k += 64) s_dst[k] = dst[k];
  __syncthreads();
  const size_t i = gtid();
  if (i >= (size_t)n) return;
  ShaLds c;
  c.blk = (uint8_t*)(lds + threadIdx.x);
  shal_init(c);
  {  // Z_pad: one all-zero block
    uint32_t z[16];
#pragma unroll
    for (int k = 0; k < 16; k++) z[k] = 0;
    sha256_compress(c.st, z);
    c.total = 64;
  }
  const uint8_t* m = msg + msg_off[i];
  const uint32_t ml = msg_len[i];
  shal_bytes(c, m, ml);
  shal_byte(c, 1);  // l_i_b_str = 256 (2 bytes, big endian)
  shal_byte(c, 0);
  shal_byte(c, 0);  // I2OSP(0, 1)
  shal_bytes(c, s_dst, dst_len);
  shal_byte(c, (uint8_t)dst_len);
  uint32_t b0[8], bi[8];
  shal_final(c, b0);
  uint32_t* o = (uint32_t*)(ub + 256 * i);
  for (int r = 1; r <= 8; r++) {
    shal_init(c);
#pragma unroll
    for (int k = 0; k < 8; k++) shal_word(c, r == 1 ? b0[k] : (b0[k] ^ bi[k]));
    shal_byte(c, (uint8_t)r);
    shal_bytes(c, s_dst, dst_len);
    shal_byte(c, (uint8_t)dst_len);
    shal_final(c, bi);
#pragma unroll
    for (int k = 0; k < 8; k++) o[8 * (r - 1) + k] = __builtin_bswap32(bi[k]);
  }
}

// stage 1: u0, u1 = hash_to_field(expand_message_xmd); norms N(tv1(u0)), N(tv1(u1)) at slots
// 2i, 2i+1 for the batched inversion
struct h2c_u_t {
  fp2_t u0, u1;
};
static_assert(lane_words<h2c_u_t>() == lsgl::W_H2CU, "layout: hash_to_field");

__global__ void LSG_KERNEL_ATTR k_h2c_prep(int n, const uint8_t* __restrict__ ub, uint32_t* __restrict__ U,
                                           uint32_t* __restrict__ norms) {
  LANE_ITEM(n);
  (void)lead;
  const uint8_t* b = ub + 256 * item;
  h2c_u_t u;
  u.u0 = fp2_make(fp_from_be64_mod(b), fp_from_be64_mod(b + 64));
  u.u1 = fp2_make(fp_from_be64_mod(b + 128), fp_from_be64_mod(b + 192));
  lane_store(U, item, u);
  lane_store(norms, 2 * item, fp2_norm(sswu_tv1(u.u0)));
  lane_store(norms, 2 * item + 1, fp2_norm(sswu_tv1(u.u1)));
}

// stage 2: SSWU -> 3-isogeny for one field element per item (2n items: u0 and u1 of set i
// are items 2i, 2i + 1, adjacent lane pairs of one quad), then P_i = Q_2i + Q_2i+1 by the even
// item with its neighbour's point moved over by a DPP quad permutation.  One map per item
// holds no second point while the other is computed (both in one item spilled 1.2 KB per
// lane).
template <class T>
LSG_DEVI T quad_swap_pairs(const T& v) {  // lanes 4i, 4i + 1 <-> 4i + 2, 4i + 3
  constexpr int W = sizeof(T) / 4;
  uint32_t w[W];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int k = 0; k < W; k++) w[k] = pdpp<0x4E>(w[k]);  // quad_perm [2, 3, 0, 1]
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_map(int n2, const uint32_t* __restrict__ U, const uint32_t* __restrict__ ninv,
                                          uint32_t* __restrict__ Hp) {
  LANE_ITEM(n2);  // n2 is even: both items of a set are live or neither is
  (void)lead;
  const g2p_t q = iso_map3(map_to_curve_sswu_ni(lane_load<fp2_t>(U, item), lane_load<fp_t>(ninv, item)));
  const g2p_t o = quad_swap_pairs(q);
  if ((item & 1) == 0) lane_store(Hp, item >> 1, g2_add(q, o));
}

// The same map as three stages around the two powers of the SSWU square root, which
// k_fp_pow_lanes (lsg_k_reduce.hip) runs between them with one element per lane: pa holds a
// power's operand and pb its result, one fp_t per item (lsg_h2c.hpp sswu_stage_a / b / c).
//   a  up to gx1, gx2; pa = N(gx1)                                          then pb = pa^((p+1)/4)
//   b  sq1 and s2 from pb; the chosen x, gx (into the state's x1, gx1); pa = c   then pb = pa^((p-3)/4)
//   c  the root from c = pa and t = pb, sgn0, the isogeny, Q0 + Q1, the store
static_assert(lane_words<sswu_mid_t>() == lsgk::POW_MAP_STATE, "layout: map stage state");
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_map_a(int n2, const uint32_t* __restrict__ U, const uint32_t* __restrict__ ninv,
                                                             uint32_t* __restrict__ state, uint32_t* __restrict__ pa) {
  LANE_ITEM(n2);
  (void)lead;
  const sswu_mid_t m = sswu_stage_a(lane_load<fp2_t>(U, item), lane_load<fp_t>(ninv, item));
  lane_store(state, item, m);
  lane_store(pa, item, fp2_norm(m.gx1));
}
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_map_b(int n2, const uint32_t* __restrict__ U, uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ pa, const uint32_t* __restrict__ pb) {
  LANE_ITEM(n2);
  (void)lead;
  sswu_mid_t m = lane_load<sswu_mid_t>(state, item);
  fp2_t x, gx;
  const fp_t c = sswu_stage_b(x, gx, m, lane_load<fp2_t>(U, item), lane_load<fp_t>(pa, item), lane_load<fp_t>(pb, item));
  m.x1 = x;
  m.gx1 = gx;
  lane_store(state, item, m);
  lane_store(pa, item, c);
}
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_map_c(int n2, const uint32_t* __restrict__ U, const uint32_t* __restrict__ state,
                                                             const uint32_t* __restrict__ pa, const uint32_t* __restrict__ pb,
                                                             uint32_t* __restrict__ Hp) {
  LANE_ITEM(n2);  // n2 is even (k_h2c_map)
  (void)lead;
  const sswu_mid_t m = lane_load<sswu_mid_t>(state, item);
  const g2p_t q = iso_map3(sswu_stage_c(lane_load<fp2_t>(U, item), m.x1, m.gx1, lane_load<fp_t>(pa, item),
                                        lane_load<fp_t>(pb, item)));
  const g2p_t o = quad_swap_pairs(q);
  if ((item & 1) == 0) lane_store(Hp, item >> 1, g2_add(q, o));
}

// stage 2b: clear_cofactor in place; zN_i = N(Z) (0 at infinity) for the batched inversion.
// The [x] chains take their base point from an LDS slot per lane and the partial sum waits in
// the item's own slot of Hp, so the chains hold only their accumulator.
// LANES: the doublings of the two chains in the component-per-lane Fp2 layout (lsg_fp2_lanes.hpp).
// The additions stay in the pair form: with them in the lane layout as well, as k_sig_subgroup
// runs them, this kernel needed 32 to 64 bytes of scratch per lane at 2 waves per SIMD.
template <bool LANES>
LSG_DEVI void h2c_clear_item(uint32_t* park, int n, uint32_t* __restrict__ Hp, uint32_t* __restrict__ zN,
                             uint8_t* __restrict__ hinf) {
  LANE_ITEM(n);
  lds_park(park, lane_load<g2p_t>(Hp, item));
  g2p_t q = clear_cofactor_g2_parked<LANES>([&]() { return lds_unpark<g2p_t>(park); },
                                            [&](const g2p_t& v) { lds_park(park, v); },
                                            [&](const g2p_t& v) { lane_store(Hp, item, v); },
                                            [&]() { return lane_load<g2p_t>(Hp, item); });
  bool is_inf = proj_is_inf(q);
  lane_store(Hp, item, q);
  lane_store(zN, item, is_inf ? fp_zero() : fp2_norm(q.Z));
  if (lead) hinf[item] = is_inf ? 1 : 0;
}
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_clear(int n, uint32_t* __restrict__ Hp, uint32_t* __restrict__ zN,
                                            uint8_t* __restrict__ hinf) {
  __shared__ uint32_t park[sizeof(g2p_t) / 4 * LSG_TPB];
  h2c_clear_item<true>(park, n, Hp, zN, hinf);
}
#ifdef LSG_FP2_LANES
// the same kernel on the pair form: the A/B library's LSG_FP2_LANES=0 and the device tests
__global__ void LSG_KERNEL_ATTR_W(LSG_H2C_WAVES) k_h2c_clear_pair(int n, uint32_t* __restrict__ Hp,
                                                                  uint32_t* __restrict__ zN, uint8_t* __restrict__ hinf) {
  __shared__ uint32_t park[sizeof(g2p_t) / 4 * LSG_TPB];
  h2c_clear_item<false>(park, n, Hp, zN, hinf);
}
#endif

// each set's hashed point from its message's (packages whose sets share messages hash every
// distinct message once)
__global__ void LSG_KERNEL_ATTR k_h2c_gather(int n, const uint32_t* __restrict__ mid, const uint32_t* __restrict__ Hm,
                                             const uint8_t* __restrict__ hinfm, uint32_t* __restrict__ H,
                                             uint8_t* __restrict__ hinf) {
  LANE_ITEM(n);
  const uint32_t m = mid[item];
  lane_store(H, item, lane_load<g2a_t>(Hm, m));
  if (lead) hinf[item] = hinfm[m];
}

// The message cache (lsg_msg_cache_set; lsg_msg_cache.hpp).  src[m] names where
// distinct message m's point is: row r of the device's arena (LSG_MC_ROW | r: a hit) or hashed
// message k of this package (k: a miss, hashed into Hx).  Words out of range copy nothing.
__global__ void LSG_KERNEL_ATTR k_h2c_cache_merge(int nm, const uint32_t* __restrict__ src, uint32_t n_rows,
                                                  const uint32_t* __restrict__ rows, const uint8_t* __restrict__ rinf,
                                                  uint32_t n_miss, const uint32_t* __restrict__ Hx,
                                                  const uint8_t* __restrict__ hinfx, uint32_t* __restrict__ Hm,
                                                  uint8_t* __restrict__ hinfm) {
  LANE_ITEM(nm);
  const uint32_t w = src[item], k = w & ~LSG_MC_ROW;
  const bool hit = (w & LSG_MC_ROW) != 0;
  if (k >= (hit ? n_rows : n_miss)) return;
  lane_store(Hm, item, lane_load<g2a_t>(hit ? rows : Hx, k));
  if (lead) hinfm[item] = hit ? rinf[k] : hinfx[k];
}

// the misses the host allotted a row to: item j copies hashed message list[2j] into row list[2j + 1]
__global__ void LSG_KERNEL_ATTR k_h2c_cache_store(int n, const uint32_t* __restrict__ list, uint32_t n_miss,
                                                  const uint32_t* __restrict__ Hx, const uint8_t* __restrict__ hinfx,
                                                  uint32_t n_rows, uint32_t* __restrict__ rows,
                                                  uint8_t* __restrict__ rinf) {
  LANE_ITEM(n);
  const uint32_t k = list[2 * item], r = list[2 * item + 1];
  if (k >= n_miss || r >= n_rows) return;
  lane_store(rows, r, lane_load<g2a_t>(Hx, k));
  if (lead) rinf[r] = hinfx[k];
}

// stage 3: H affine = (X, Y) * conj(Z) / N(Z)   (= proj_to_aff, 1/Z = conj(Z) / N(Z))
__global__ void LSG_KERNEL_ATTR k_h2c_affine(int n, const uint32_t* __restrict__ Hp, const uint32_t* __restrict__ ninv,
                                             const uint8_t* __restrict__ hinf, uint32_t* __restrict__ H) {
  LANE_ITEM(n);
  (void)lead;
  g2p_t q = lane_load<g2p_t>(Hp, item);
  g2a_t a;
  if (hinf[item]) {
    a.x = fp2_zero();
    a.y = fp2_zero();
  } else {
    fp2_t zi = fp2_inv_with_norm_inv(q.Z, lane_load<fp_t>(ninv, item));
    a.x = fp2_mul(q.X, zi);
    a.y = fp2_mul(q.Y, zi);
  }
  lane_store(H, item, a);
}

// ---- SSZ signing roots, one thread per object: the trees are the
// functions of lsg_ssz.hpp (hash_tree_root(SigningData{objectRoot, domain}),
// util/signingRoot.ts:7-13), which tests/native/sszcheck.cpp runs on the CPU.
__global__ void __launch_bounds__(64) k_signing_root(int n, const uint8_t* __restrict__ roots,
                                                     const uint8_t* __restrict__ domains, uint32_t dstride,
                                                     uint8_t* __restrict__ out32) {
  size_t i = gtid();
  if (i >= (size_t)n) return;
  ssz_signing_root_chunk(roots + 32 * i, 32, domains + dstride * i, out32 + 32 * i);
}

// getAttestationDataSigningRoot (signatureSets/indexedAttestation.ts:11-19) from the SSZ
// serialization of phase0.AttestationData (128 bytes)
__global__ void __launch_bounds__(64) k_attestation_signing_root(int n, const uint8_t* __restrict__ data,
                                                                 const uint8_t* __restrict__ domains,
                                                                 uint32_t dstride, uint8_t* __restrict__ out32) {
  size_t i = gtid();
  if (i >= (size_t)n) return;
  ssz_signing_root_attestation(data + 128 * i, domains + dstride * i, out32 + 32 * i);
}

// computeSigningRoot(ssz.phase0.DepositMessage, msg, domain) (block/processDeposit.ts:49-54)
// from the SSZ serialization of DepositMessage (88 bytes) at data + stride i (stride 184: the
// head of a DepositData)
__global__ void __launch_bounds__(64) k_deposit_signing_root(int n, const uint8_t* __restrict__ data, uint32_t stride,
                                                             const uint8_t* __restrict__ domains, uint32_t dstride,
                                                             uint8_t* __restrict__ out32) {
  size_t i = gtid();
  if (i >= (size_t)n) return;
  ssz_signing_root_deposit(data + (size_t)stride * i, domains + dstride * i, out32 + 32 * i);
}

// any kind of lsg_object_signing_roots: n objects of obj_len bytes back to back
__global__ void __launch_bounds__(64) k_object_signing_root(int n, const uint8_t* __restrict__ objs, uint32_t obj_len,
                                                            const uint8_t* __restrict__ domains, uint32_t dstride,
                                                            uint8_t* __restrict__ out32) {
  size_t i = gtid();
  if (i >= (size_t)n) return;
  ssz_object_signing_root(obj_len, objs + (size_t)obj_len * i, domains + dstride * i, out32 + 32 * i);
}

// First stage of a package with LSG_MSG_OBJECT sets, one thread per distinct
// staged message.  A message whose staged length carries the marker is an SSZ object followed
// by its domain: its signing root goes over the first 32 bytes of its own payload (payloads
// are disjoint and at least 40 bytes; the root is stored after the whole payload is read) and
// its length word becomes 32, so k_expand_msg finds an ordinary 32-byte message.  Unmarked
// messages are left alone.  The stager admits only the payload lengths of the table
// (lsgp::msg_object_kind); another one would leave an empty message.
__global__ void __launch_bounds__(64) k_msg_roots(int n, uint8_t* msg, const uint32_t* __restrict__ msg_off,
                                                  uint32_t* __restrict__ msg_len) {
  size_t i = gtid();
  if (i >= (size_t)n) return;
  const uint32_t l = msg_len[i];
  if (!(l & LSG_MSG_OBJECT) || (l & LSG_MSG_KIND_MASK)) return;  // (tagged messages: k_msg_roots_var)
  const uint32_t obj_len = (l & ~LSG_MSG_OBJECT) - 32u;
  uint8_t* p = msg + msg_off[i];
  msg_len[i] = ssz_object_signing_root(obj_len, p, p + obj_len, p) ? 32u : 0u;
}

// The variable-size kinds (a non-zero kind tag in the staged length word: AggregateAndProof,
// DESIGN.md 5j), one 64-lane workgroup per staged message; a workgroup whose message carries no
// tag leaves at once.  The lanes run the phases of lsg_ssz.hpp's ssz_var_step -- pairs of one
// tree level side by side, the fixed part's subtrees on lanes of their own -- with the
// intermediate nodes in LDS (12,384 bytes) and a barrier after each phase, so an object costs
// about depth + chunks / 128 dependent node hashes, not one per chunk.  Payloads have no
// alignment: byte loads.  out32 == null (a package): the root goes over the start of the
// payload, stored by lane 0 in the last phase, after every read, and the length word becomes
// 32 as in k_msg_roots.  out32 != null (lsg_object_signing_roots_var): root m at out32 + 32 m,
// the payload and its length word left alone.  The stager admits only well-formed objects
// (lsgp::msg_var_ok); a length that would leave the node buffer leaves an empty message.
__global__ void __launch_bounds__(SSZ_VAR_LANES) k_msg_roots_var(int n, uint8_t* msg, const uint32_t* __restrict__ msg_off,
                                                                 uint32_t* msg_len, uint8_t* out32) {
  __shared__ uint32_t nodes[SSZ_VAR_NODE_WORDS];
  const uint32_t m = blockIdx.x, lane = threadIdx.x;
  if (m >= (uint32_t)n) return;
  const uint32_t l = msg_len[m];
  const uint32_t kind = (l & LSG_MSG_KIND_MASK) >> LSG_MSG_KIND_SHIFT;
  if (!(l & LSG_MSG_OBJECT) || kind == 0) return;
  const uint32_t payload = l & ~(LSG_MSG_OBJECT | LSG_MSG_KIND_MASK);
  uint8_t* p = msg + msg_off[m];
  uint8_t* out = out32 ? out32 + 32 * (size_t)m : p;
  const bool in_range = kind <= 2 && payload > 32 + ssz_var_bits_off(kind) &&
                        payload <= 32 + ssz_var_bits_off(kind) + ssz_var_max_bits(kind) / 8 + 1;
  const uint32_t obj_len = payload - 32;
  const SszVar v = ssz_var_shape(kind, in_range ? obj_len : ssz_var_bits_off(kind) + 1, in_range ? p[obj_len - 1] : 1);
  if (!in_range || v.n_bits > ssz_var_max_bits(kind)) {  // (uniform over the workgroup)
    __syncthreads();  // every lane has read the length word
    if (lane == 0 && !out32) msg_len[m] = 0;
    return;
  }
  const uint32_t phases = ssz_var_phases(v);
  for (uint32_t ph = 0; ph < phases; ph++) {
    ssz_var_step(v, ph, lane, p, p + obj_len, nodes, out);
    __syncthreads();
  }
  if (lane == 0 && !out32) msg_len[m] = 32;
}

namespace lsgk {
hipError_t deposit_signing_root(hipStream_t st, int n, const uint8_t* data, uint32_t stride, const uint8_t* domains,
                                uint32_t dstride, uint8_t* out32) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_deposit_signing_root, dim3((n + 63) / 64), dim3(64), 0, st, n, data, stride, domains, dstride,
                     out32);
  return hipGetLastError();
}
hipError_t object_signing_root(hipStream_t st, int n, const uint8_t* objs, uint32_t obj_len, const uint8_t* domains,
                               uint32_t dstride, uint8_t* out32) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_object_signing_root, dim3((n + 63) / 64), dim3(64), 0, st, n, objs, obj_len, domains, dstride,
                     out32);
  return hipGetLastError();
}
hipError_t msg_roots(hipStream_t st, int n, uint8_t* msg, const uint32_t* off, uint32_t* len) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_msg_roots, dim3((n + 63) / 64), dim3(64), 0, st, n, msg, off, len);
  return hipGetLastError();
}
hipError_t msg_roots_var(hipStream_t st, int n, uint8_t* msg, const uint32_t* off, uint32_t* len, uint8_t* out32) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_msg_roots_var, dim3(n), dim3(SSZ_VAR_LANES), 0, st, n, msg, off, len, out32);
  return hipGetLastError();
}
hipError_t expand_msg(hipStream_t st, int n, const uint8_t* msg, const uint32_t* off, const uint32_t* len,
                      const uint8_t* dst, uint32_t dst_len, uint8_t* ub) {
  if (n <= 0) return hipSuccess;
  if (dst_len > 255) return hipErrorInvalidValue;  // the kernel's LDS copy (RFC 9380: DST < 256 bytes)
  hipLaunchKernelGGL(k_expand_msg, dim3((n + 63) / 64), dim3(64), 0, st, n, msg, off, len, dst, dst_len, ub);
  return hipGetLastError();
}
hipError_t h2c_prep(hipStream_t st, int n, const uint8_t* ub, uint32_t* U, uint32_t* norms) {
  LSG_LAUNCH_ITEMS(k_h2c_prep, n, st, n, ub, U, norms);
}
hipError_t h2c_map(hipStream_t st, int n, const uint32_t* U, const uint32_t* ninv, uint32_t* Hp, const PowLanes& pw) {
  if (n <= 0) return hipSuccess;
  const int n2 = 2 * n;
  if (!pw.on(n2)) LSG_LAUNCH_ITEMS(k_h2c_map, n2, st, n2, U, ninv, Hp);
  const dim3 grid(lane_blocks((size_t)n2)), block(LSG_TPB);
  hipLaunchKernelGGL(k_h2c_map_a, grid, block, 0, st, n2, U, ninv, pw.state, pw.pa);
  hipError_t e = fp_pow_lanes(st, n2, LSG_POW_SQRT, pw.pa, pw.pb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_h2c_map_b, grid, block, 0, st, n2, U, pw.state, pw.pa, pw.pb);
  e = fp_pow_lanes(st, n2, LSG_POW_SQRT34, pw.pa, pw.pb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_h2c_map_c, grid, block, 0, st, n2, U, pw.state, pw.pa, pw.pb, Hp);
  return hipGetLastError();
}
hipError_t h2c_clear(hipStream_t st, int n, uint32_t* Hp, uint32_t* zN, uint8_t* hinf, bool pair_form) {
#ifdef LSG_FP2_LANES
  if (pair_form) LSG_LAUNCH_ITEMS(k_h2c_clear_pair, n, st, n, Hp, zN, hinf);
#endif
  (void)pair_form;
  LSG_LAUNCH_ITEMS(k_h2c_clear, n, st, n, Hp, zN, hinf);
}
hipError_t h2c_gather(hipStream_t st, int n, const uint32_t* mid, const uint32_t* Hm, const uint8_t* hinfm, uint32_t* H,
                      uint8_t* hinf) {
  LSG_LAUNCH_ITEMS(k_h2c_gather, n, st, n, mid, Hm, hinfm, H, hinf);
}
hipError_t h2c_cache_merge(hipStream_t st, int nm, const uint32_t* src, uint32_t n_rows, const uint32_t* rows,
                           const uint8_t* rinf, uint32_t n_miss, const uint32_t* Hx, const uint8_t* hinfx, uint32_t* Hm,
                           uint8_t* hinfm) {
  LSG_LAUNCH_ITEMS(k_h2c_cache_merge, nm, st, nm, src, n_rows, rows, rinf, n_miss, Hx, hinfx, Hm, hinfm);
}
hipError_t h2c_cache_store(hipStream_t st, int n, const uint32_t* list, uint32_t n_miss, const uint32_t* Hx,
                           const uint8_t* hinfx, uint32_t n_rows, uint32_t* rows, uint8_t* rinf) {
  LSG_LAUNCH_ITEMS(k_h2c_cache_store, n, st, n, list, n_miss, Hx, hinfx, n_rows, rows, rinf);
}
hipError_t h2c_affine(hipStream_t st, int n, const uint32_t* Hp, const uint32_t* ninv, const uint8_t* hinf,
                      uint32_t* H) {
  LSG_LAUNCH_ITEMS(k_h2c_affine, n, st, n, Hp, ninv, hinf, H);
}
hipError_t signing_root(hipStream_t st, int n, const uint8_t* roots, const uint8_t* domains, uint32_t dstride,
                        uint8_t* out32) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_signing_root, dim3((n + 63) / 64), dim3(64), 0, st, n, roots, domains, dstride, out32);
  return hipGetLastError();
}
hipError_t attestation_signing_root(hipStream_t st, int n, const uint8_t* data, const uint8_t* domains,
                                    uint32_t dstride, uint8_t* out32) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_attestation_signing_root, dim3((n + 63) / 64), dim3(64), 0, st, n, data, domains, dstride,
                     out32);
  return hipGetLastError();
}
}  // namespace lsgk
