// lsg_k_sig.hip -- signature kernels: Signature.fromBytes(sig, affine, validate=true)
// (packages/beacon-node/src/chain/bls/maybeBatch.ts:23,36), the points each
// set adds to its group's RLC signature sum (blst mul_n_aggregate; 8a M4), G2 serialisation
// and the test/bench signer.
#include "lsg_kcommon.hpp"

__global__ void LSG_KERNEL_ATTR k_sig_decode(int n, const uint8_t* __restrict__ sig, const uint32_t* __restrict__ sig_len,
                                             uint32_t* __restrict__ sig_aff, uint8_t* __restrict__ inf,
                                             int32_t* __restrict__ err) {
  LANE_ITEM(n);
  uint32_t len = sig_len[item];
  g2a_t p;
  p.x = fp2_zero();
  p.y = fp2_zero();
  bool is_inf = false;
  int e;
  if (len == 96)
    e = g2_uncompress(p, is_inf, sig + 192 * item);
  else if (len == 192)
    e = g2_deserialize_uncompressed(p, is_inf, sig + 192 * item);
  else
    e = LSG_BLST_INVALID_SIZE;
  lane_store(sig_aff, item, p);
  if (lead) {
    inf[item] = is_inf ? 1 : 0;
    err[item] = e;
  }
}

// The same decode as three stages around the two powers of the square root, which
// k_fp_pow_lanes (lsg_k_reduce.hip) runs between them with one element per lane: pa holds a
// power's operand and pb its result, one fp_t per item.
//   a  parse; rhs = x^3 + b; pa = N(rhs)                                 then pb = pa^((p+1)/4)
//   b  ok = (pb^2 == pa); pa = c (fp2_sqrt_root_c)                       then pb = pa^((p-3)/4)
//   c  the root from c = pa and t = pb, the curve check, the sign, the store
// Only a well-formed 96-byte encoding reaches the root (state word bit 0): every other item --
// wrong size, flag errors, infinity, the 192-byte form -- is finished by stage a with the code and
// precedence of k_sig_decode, sends 0 through the powers and is skipped by b and c.
struct sigdec_state_t {
  fp2_t x, rhs;
  uint32_t w;  // bit 0: at the root, 1: the sign flag, 2: N(rhs) is a square (stage b)
};
static_assert(lane_words<sigdec_state_t>() == lsgk::POW_SIG_STATE, "layout: decode stage state");
__global__ void LSG_KERNEL_ATTR k_sig_decode_a(int n, const uint8_t* __restrict__ sig, const uint32_t* __restrict__ sig_len,
                                               uint32_t* __restrict__ sig_aff, uint8_t* __restrict__ inf,
                                               int32_t* __restrict__ err, uint32_t* __restrict__ state,
                                               uint32_t* __restrict__ pa) {
  LANE_ITEM(n);
  uint32_t len = sig_len[item];
  g2a_t p;
  p.x = fp2_zero();
  p.y = fp2_zero();
  sigdec_state_t s;
  s.x = fp2_zero();
  s.rhs = fp2_zero();
  s.w = 0;
  fp_t pw = fp_zero();
  bool is_inf = false;
  int e;
  if (len == 96) {
    bool want = false;
    e = g2_uncompress_parse(p, is_inf, s.x, s.rhs, want, sig + 192 * item);
    if (e == LSG_UNCOMPRESS_PENDING) {
      s.w = 1u | (want ? 2u : 0u);
      pw = fp2_norm(s.rhs);
    }
  } else if (len == 192)
    e = g2_deserialize_uncompressed(p, is_inf, sig + 192 * item);
  else
    e = LSG_BLST_INVALID_SIZE;
  lane_store(state, item, s);
  lane_store(pa, item, pw);
  if (e == LSG_UNCOMPRESS_PENDING) return;
  lane_store(sig_aff, item, p);
  if (lead) {
    inf[item] = is_inf ? 1 : 0;
    err[item] = e;
  }
}
__global__ void LSG_KERNEL_ATTR k_sig_decode_b(int n, uint32_t* __restrict__ state, uint32_t* __restrict__ pa,
                                               const uint32_t* __restrict__ pb) {
  LANE_ITEM(n);
  (void)lead;
  sigdec_state_t s = lane_load<sigdec_state_t>(state, item);
  if (!(s.w & 1u)) return;
  const fp_t cand = lane_load<fp_t>(pb, item);
  if (fp_is_root_of(cand, lane_load<fp_t>(pa, item))) s.w |= 4u;
  lane_store(pa, item, fp2_sqrt_root_c(s.rhs, cand));
  lane_store(state, item, s);
}
__global__ void LSG_KERNEL_ATTR k_sig_decode_c(int n, const uint32_t* __restrict__ state, const uint32_t* __restrict__ pa,
                                               const uint32_t* __restrict__ pb, uint32_t* __restrict__ sig_aff,
                                               uint8_t* __restrict__ inf, int32_t* __restrict__ err) {
  LANE_ITEM(n);
  const sigdec_state_t s = lane_load<sigdec_state_t>(state, item);
  if (!(s.w & 1u)) return;
  fp2_t y;
  const bool root = fp2_sqrt_root_finish(y, s.rhs, lane_load<fp_t>(pa, item), lane_load<fp_t>(pb, item));
  g2a_t p;
  p.x = fp2_zero();
  p.y = fp2_zero();
  const int e = g2_uncompress_finish(p, s.x, y, (s.w & 4u) != 0 && root, (s.w & 2u) != 0);
  lane_store(sig_aff, item, p);
  if (lead) {
    inf[item] = 0;
    err[item] = e;
  }
}

// psi(P) == [x]P (Jacobian doubling chain, complete additions); the chain's base point waits
// in an LDS slot per lane, re-read at the five additions, instead of in spilled registers
// F: the layout the chain runs in and the point is parked in (chain_fp2_t: one Fp2 component
// per lane, lsg_fp2_lanes.hpp); sig_aff is read in the pair form and converted at the load
template <class F>
LSG_DEVI void sig_subgroup_item(uint32_t* park, int n, const uint32_t* __restrict__ sig_aff,
                                const uint8_t* __restrict__ inf, int32_t* __restrict__ err) {
  LANE_ITEM(n);
  if (err[item] != 0 || inf[item]) return;
  lds_park(park, g2_layout<F>::in(lane_load<g2a_t>(sig_aff, item)));
  // the parked point is affine and finite: the chain's five additions are mixed ones
  bool ok = g2_in_group_get<F>([&]() { return lds_unpark<aff_t<F>>(park); });
  if (lead && !ok) err[item] = LSG_BLST_POINT_NOT_IN_GROUP;
}
__global__ void LSG_KERNEL_ATTR k_sig_subgroup(int n, const uint32_t* __restrict__ sig_aff,
                                               const uint8_t* __restrict__ inf, int32_t* __restrict__ err) {
  __shared__ uint32_t park[sizeof(g2a_t) / 4 * LSG_TPB];
  sig_subgroup_item<chain_fp2_t>(park, n, sig_aff, inf, err);
}
#ifdef LSG_FP2_LANES
// the same kernel on the pair form: the A/B library's LSG_FP2_LANES=0 and the device tests
__global__ void LSG_KERNEL_ATTR k_sig_subgroup_pair(int n, const uint32_t* __restrict__ sig_aff,
                                                    const uint8_t* __restrict__ inf, int32_t* __restrict__ err) {
  __shared__ uint32_t park[sizeof(g2a_t) / 4 * LSG_TPB];
  sig_subgroup_item<fp2_t>(park, n, sig_aff, inf, err);
}
#endif

// The point set i adds to its group's signature sum S_g = sum r_i sig_i: the identity for a
// set that cannot contribute (undecodable or infinite signature, infinite aggregated key: the
// verdict rules exclude such sets, lsg_host.hip), else sig_i (k_sig_proj: bucket MSM groups
// scale later) or [r_i] sig_i (k_sig_scale3: groups below the MSM threshold, sets whose mode
// byte is set).  Two kernels, so that the MSM path never carries the scaled path's window
// table.
LSG_DEVI bool sig_usable(size_t i, const uint8_t* inf, const int32_t* err, const uint8_t* pinf) {
  return err[i] == 0 && !inf[i] && !(pinf && pinf[i]);
}
__global__ void LSG_KERNEL_ATTR k_sig_proj(int n, const uint32_t* __restrict__ sig_aff, const uint8_t* __restrict__ inf,
                                           const int32_t* __restrict__ err, const uint8_t* __restrict__ pinf,
                                           uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  g2p_t r = proj_inf<fp2_t>();
  if (sig_usable(item, inf, err, pinf)) r = proj_from_aff(lane_load<g2a_t>(sig_aff, item));
  lane_store(out, item, r);
}
// [r_i] sig_i with signed 3-bit windows (65 doublings + 22 additions, the window table in
// 512 registers at 1 wave per SIMD, no scratch; 4-bit windows with the table in scratch were
// measured slower: profiles/r03_*_scale3ab.json)
__global__ void LSG_KERNEL_ATTR_W(1) k_sig_scale3(int n, const uint32_t* __restrict__ sig_aff, const uint8_t* __restrict__ inf,
                                                  const int32_t* __restrict__ err, const uint8_t* __restrict__ pinf,
                                                  const uint64_t* __restrict__ rnd, const uint8_t* __restrict__ mode,
                                                  uint32_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  if (mode && !mode[item]) return;  // a set of an MSM group: k_sig_proj wrote its point
  g2p_t r = proj_inf<fp2_t>();
  if (sig_usable(item, inf, err, pinf)) {
    r = proj_from_aff(lane_load<g2a_t>(sig_aff, item));
    if (rnd[item] != 0) r = proj_mul_u64_s3(r, rnd[item]);  // r_i = 0: a set verified alone, not scaled
  }
  lane_store(out, item, r);
}

// Signature.aggregate of the verified signatures per caller-named group (lsg_submit_jobs_grouped;
// SURVEY.md 8f(7)): the G2 twin of k_pk_agg_seg (lsg_k_pk.hip).  One pass of the segmented
// reduction (lsg_plan.hpp plan_sig_groups) whose elements are the decoded, subgroup-checked
// affine signatures already resident in sig_aff, reached through the gather list (set slots
// ordered by group) and folded with complete mixed additions -- no projective copy of every
// signature written and read back -- then the chunk's lane pairs combined by a butterfly.
// Chunk = (first list entry, count, output: >= 0 into dst, < 0 into tmp for k_seg_reduce<1>).
// A set that is not usable (err != 0 or the point at infinity) adds nothing.
__global__ void LSG_KERNEL_ATTR k_sig_agg_seg(int n_chunks, int ips_log2, const int32_t* __restrict__ chunks,
                                              const int32_t* __restrict__ gather, const uint32_t* __restrict__ sig_aff,
                                              const uint8_t* __restrict__ inf, const int32_t* __restrict__ err,
                                              uint32_t* __restrict__ dst, uint32_t* __restrict__ tmp) {
  lsg_lane_setup();
  const size_t item = gtid() / LSG_GROUP;
  const size_t c = item >> ips_log2;
  const int ips = 1 << ips_log2, j = (int)(item & (size_t)(ips - 1));
  const bool active = c < (size_t)n_chunks;
  g2p_t acc = proj_inf<fp2_t>();
  int out = 0;
  if (active) {
    const int off = chunks[3 * c], len = chunks[3 * c + 1];
    out = chunks[3 * c + 2];
    // software-pipelined as k_pk_agg_seg: the next signature's row is in flight while this one
    // is added (the gathers are scattered over the package's sets)
    g2a_t a;
    bool use = false;
    auto fetch = [&](int k) {
      const size_t i = (size_t)gather[off + k];
      a = lane_load<g2a_t>(sig_aff, i);
      return sig_usable(i, inf, err, nullptr);
    };
    if (j < len) use = fetch(j);
#pragma unroll 1
    for (int k = j; k < len; k += ips) {
      const g2a_t cur = a;
      const bool cur_use = use;
      if (k + ips < len) use = fetch(k + ips);
      if (cur_use) acc = proj_is_inf(acc) ? proj_from_aff(cur) : g2_add_mixed(acc, cur);
    }
  }
  // every lane runs the butterfly: a chunk never straddles a wave (ips <= 32 pairs)
#pragma unroll 1
  for (int o = ips >> 1; o >= 1; o >>= 1) acc = g2_add(acc, shfl_xor_t(acc, LSG_GROUP * o));
  if (active && j == 0) {
    if (out >= 0)
      lane_store(dst, (size_t)out, acc);
    else
      lane_store(tmp, (size_t)(-out - 1), acc);
  }
}

// The bucket pass of the signature MSM (plan_phase / plan_buckets, lsg_plan.hpp): bucket (w, d) =
// the sum of the sets whose w-th digit of r_i is d, over the resident affine signatures -- the
// gather of k_sig_agg_seg with the skip rule of k_sig_proj (sig_usable: an unusable set adds
// nothing), so no projective copy of every signature is written and read back once per window.
// Each lane pair folds its members serially with mixed additions (g2_fold_mixed, lsg_curve.hpp)
// in the layout F -- one Fp2 component per lane, or the pair form -- and the chunk's pairs are
// combined in the pair form by the butterfly of complete additions.  The plan gives a chunk few
// pairs (the pass is work-bound: a butterfly level costs every pair one addition, of which half,
// three quarters, ... are thrown away), so most of the work is the fold.
template <class F>
LSG_DEVI void msm_bucket_item(int n_chunks, int ips_log2, const int32_t* __restrict__ chunks,
                              const int32_t* __restrict__ gather, const uint32_t* __restrict__ sig_aff,
                              const uint8_t* __restrict__ inf, const int32_t* __restrict__ err,
                              const uint8_t* __restrict__ pinf, uint32_t* __restrict__ dst, uint32_t* __restrict__ tmp) {
  lsg_lane_setup();
  const size_t item = gtid() / LSG_GROUP;
  const size_t c = item >> ips_log2;
  const int ips = 1 << ips_log2, j = (int)(item & (size_t)(ips - 1));
  const bool active = c < (size_t)n_chunks;
  g2p_t acc = proj_inf<fp2_t>();
  int out = 0;
  if (active) {
    const int off = chunks[3 * c], len = chunks[3 * c + 1];
    out = chunks[3 * c + 2];
    acc = g2_to_pair(g2_fold_mixed<F>(j, ips, len, [&](int k, g2a_t& a) {
      const size_t i = (size_t)gather[off + k];
      a = lane_load<g2a_t>(sig_aff, i);
      return sig_usable(i, inf, err, pinf);
    }));
  }
  // every lane runs the butterfly: a chunk never straddles a wave (ips <= 32 pairs)
#pragma unroll 1
  for (int o = ips >> 1; o >= 1; o >>= 1) acc = g2_add(acc, shfl_xor_t(acc, LSG_GROUP * o));
  if (active && j == 0) {
    if (out >= 0)
      lane_store(dst, (size_t)out, acc);
    else
      lane_store(tmp, (size_t)(-out - 1), acc);
  }
}
__global__ void LSG_KERNEL_ATTR k_msm_bucket_seg(int n_chunks, int ips_log2, const int32_t* __restrict__ chunks,
                                                 const int32_t* __restrict__ gather, const uint32_t* __restrict__ sig_aff,
                                                 const uint8_t* __restrict__ inf, const int32_t* __restrict__ err,
                                                 const uint8_t* __restrict__ pinf, uint32_t* __restrict__ dst,
                                                 uint32_t* __restrict__ tmp) {
  msm_bucket_item<chain_fp2_t>(n_chunks, ips_log2, chunks, gather, sig_aff, inf, err, pinf, dst, tmp);
}
#ifdef LSG_FP2_LANES
// the same kernel with its fold in the pair form: the A/B library's LSG_FP2_LANES=0 and the device tests
__global__ void LSG_KERNEL_ATTR k_msm_bucket_seg_pair(int n_chunks, int ips_log2, const int32_t* __restrict__ chunks,
                                                      const int32_t* __restrict__ gather,
                                                      const uint32_t* __restrict__ sig_aff, const uint8_t* __restrict__ inf,
                                                      const int32_t* __restrict__ err, const uint8_t* __restrict__ pinf,
                                                      uint32_t* __restrict__ dst, uint32_t* __restrict__ tmp) {
  msm_bucket_item<fp2_t>(n_chunks, ips_log2, chunks, gather, sig_aff, inf, err, pinf, dst, tmp);
}
#endif

__global__ void LSG_KERNEL_ATTR k_g2a_to_bytes(int n, const uint32_t* __restrict__ pts, const uint8_t* __restrict__ inf,
                                               uint8_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  g2_serialize(out + 192 * item, lane_load<g2a_t>(pts, item), inf[item] != 0);
}

// projective G2 -> ZCash-compressed 96 bytes (Signature.toBytes(); the identity -> 0xc0 || 0^95)
__global__ void LSG_KERNEL_ATTR k_g2p_compress(int n, const uint32_t* __restrict__ pts, uint8_t* __restrict__ out96) {
  LANE_ITEM(n);
  (void)lead;
  g2p_t p = lane_load<g2p_t>(pts, item);
  bool is_inf = proj_is_inf(p);
  g2a_t a;
  if (is_inf) {
    a.x = fp2_zero();
    a.y = fp2_zero();
  } else {
    a = proj_to_aff(p);
  }
  g2_compress(out96 + 96 * item, a, is_inf);
}

// projective G2 (lane form) -> canonical 288-byte blobs for the per-group programs (lsg_slp.hip)
__global__ void LSG_KERNEL_ATTR k_g2p_to_canon(int n, const uint32_t* __restrict__ in, uint8_t* __restrict__ out) {
  LANE_ITEM(n);
  (void)lead;
  g2p_to_canon_bytes(out + 288 * item, lane_load<g2p_t>(in, item));
}

// [k]P for a 256-bit big-endian scalar (test-data utilities only: signing, keygen)
template <class F>
__device__ proj_t<F> proj_mul_be256(const proj_t<F>& p, const uint8_t* k) {
  proj_t<F> acc = proj_inf<F>();
  for (int byte = 0; byte < 32; byte++) {
    uint32_t v = k[byte];
    for (int b = 7; b >= 0; b--) {
      acc = gdbl(acc);
      proj_t<F> s = gadd(acc, p);
      bool bit = (v >> b) & 1u;
      acc.X = fselect(bit, s.X, acc.X);
      acc.Y = fselect(bit, s.Y, acc.Y);
      acc.Z = fselect(bit, s.Z, acc.Z);
    }
  }
  return acc;
}

// sig_i = [sk_i] H(m_i), ZCash-compressed (bench/test input generation; not on the verify path)
__global__ void LSG_KERNEL_ATTR k_sign(int n, const uint8_t* __restrict__ sks, const uint32_t* __restrict__ H,
                                       uint8_t* __restrict__ out96) {
  LANE_ITEM(n);
  (void)lead;
  g2p_t s = proj_mul_be256(proj_from_aff(lane_load<g2a_t>(H, item)), sks + 32 * item);
  bool is_inf = proj_is_inf(s);
  g2a_t a;
  if (is_inf) {
    a.x = fp2_zero();
    a.y = fp2_zero();
  } else {
    a = proj_to_aff(s);
  }
  g2_compress(out96 + 96 * item, a, is_inf);
}

namespace lsgk {
hipError_t sig_decode(hipStream_t st, int n, const uint8_t* sig, const uint32_t* sig_len, uint32_t* sig_aff,
                      uint8_t* inf, int32_t* err, const PowLanes& pw) {
  if (n <= 0) return hipSuccess;
  if (!pw.on(n)) LSG_LAUNCH_ITEMS(k_sig_decode, n, st, n, sig, sig_len, sig_aff, inf, err);
  const dim3 grid(lane_blocks((size_t)n)), block(LSG_TPB);
  hipLaunchKernelGGL(k_sig_decode_a, grid, block, 0, st, n, sig, sig_len, sig_aff, inf, err, pw.state, pw.pa);
  hipError_t e = fp_pow_lanes(st, n, LSG_POW_SQRT, pw.pa, pw.pb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sig_decode_b, grid, block, 0, st, n, pw.state, pw.pa, pw.pb);
  e = fp_pow_lanes(st, n, LSG_POW_SQRT34, pw.pa, pw.pb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sig_decode_c, grid, block, 0, st, n, pw.state, pw.pa, pw.pb, sig_aff, inf, err);
  return hipGetLastError();
}
hipError_t sig_subgroup(hipStream_t st, int n, const uint32_t* sig_aff, const uint8_t* inf, int32_t* err, bool pair_form) {
#ifdef LSG_FP2_LANES
  if (pair_form) LSG_LAUNCH_ITEMS(k_sig_subgroup_pair, n, st, n, sig_aff, inf, err);
#endif
  (void)pair_form;
  LSG_LAUNCH_ITEMS(k_sig_subgroup, n, st, n, sig_aff, inf, err);
}
hipError_t sig_prep(hipStream_t st, int n, const uint32_t* sig_aff, const uint8_t* inf, const int32_t* err,
                    const uint8_t* pinf, const uint64_t* rnd, const uint8_t* mode, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  if (!rnd || mode) {  // unscaled points for every set (mode: the scaled sets are overwritten next)
    hipLaunchKernelGGL(k_sig_proj, dim3(lane_blocks((size_t)n)), dim3(LSG_TPB), 0, st, n, sig_aff, inf, err, pinf, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !rnd) return e;
  }
  return sig_scale_only(st, n, sig_aff, inf, err, pinf, rnd, mode, out);
}
hipError_t sig_scale_only(hipStream_t st, int n, const uint32_t* sig_aff, const uint8_t* inf, const int32_t* err,
                          const uint8_t* pinf, const uint64_t* rnd, const uint8_t* mode, uint32_t* out) {
  LSG_LAUNCH_ITEMS(k_sig_scale3, n, st, n, sig_aff, inf, err, pinf, rnd, mode, out);
}
hipError_t sig_agg_seg(hipStream_t st, int n_chunks, int ips_log2, const int32_t* chunks, const int32_t* gather,
                       const uint32_t* sig_aff, const uint8_t* inf, const int32_t* err, uint32_t* dst, uint32_t* tmp) {
  LSG_LAUNCH_ITEMS(k_sig_agg_seg, (size_t)n_chunks << ips_log2, st, n_chunks, ips_log2, chunks, gather, sig_aff, inf, err,
                   dst, tmp);
}
hipError_t msm_bucket_seg(hipStream_t st, int n_chunks, int ips_log2, const int32_t* chunks, const int32_t* gather,
                          const uint32_t* sig_aff, const uint8_t* inf, const int32_t* err, const uint8_t* pinf,
                          uint32_t* dst, uint32_t* tmp, bool pair_form) {
#ifdef LSG_FP2_LANES
  if (pair_form)
    LSG_LAUNCH_ITEMS(k_msm_bucket_seg_pair, (size_t)n_chunks << ips_log2, st, n_chunks, ips_log2, chunks, gather, sig_aff,
                     inf, err, pinf, dst, tmp);
#endif
  (void)pair_form;
  LSG_LAUNCH_ITEMS(k_msm_bucket_seg, (size_t)n_chunks << ips_log2, st, n_chunks, ips_log2, chunks, gather, sig_aff, inf,
                   err, pinf, dst, tmp);
}
hipError_t g2a_to_bytes(hipStream_t st, int n, const uint32_t* pts, const uint8_t* inf, uint8_t* out192) {
  LSG_LAUNCH_ITEMS(k_g2a_to_bytes, n, st, n, pts, inf, out192);
}
hipError_t g2p_compress(hipStream_t st, int n, const uint32_t* pts, uint8_t* out96) {
  LSG_LAUNCH_ITEMS(k_g2p_compress, n, st, n, pts, out96);
}
hipError_t g2p_to_canon(hipStream_t st, int n, const uint32_t* pts, uint8_t* out288) {
  LSG_LAUNCH_ITEMS(k_g2p_to_canon, n, st, n, pts, out288);
}
hipError_t sign(hipStream_t st, int n, const uint8_t* sks, const uint32_t* H, uint8_t* out96) {
  LSG_LAUNCH_ITEMS(k_sign, n, st, n, sks, H, out96);
}
}  // namespace lsgk
