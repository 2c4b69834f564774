// Launchers of the straight-line programs (lsg_slp.hip, tools/gen_slp.py): one group per
// workgroup, each step's independent products spread over the lane pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// verdict[g] = (FE(F_g) == 1) for ng canonical 576-byte Fp12 blobs
hipError_t lsg_slp_final_exp(hipStream_t st, int ng, const uint8_t* F576, int32_t* verdict);
// out576[g] = ML(-G1, S_g) for ng canonical 288-byte projective G2 points (1 if S_g = O)
hipError_t lsg_slp_miller_neg_g1(hipStream_t st, int ng, const uint8_t* S288, uint8_t* out576);
// out576[g] = ML(-G1, sum_k 2^k C_{g,k}) for ng groups of 64 canonical 288-byte projective G2
// points each (the bucket MSM's per-bit sums): Horner and the Miller loop in one program
hipError_t lsg_slp_horner_miller(hipStream_t st, int ng, const uint8_t* C288, uint8_t* out576);
// hash_to_G2's cofactor clearing and affine conversion: Hp (projective lane form, the SSWU
// map's Q0 + Q1) -> H (affine lane form), hinf
hipError_t lsg_slp_h2c_clear(hipStream_t st, int n, const uint32_t* Hp, uint32_t* H, uint8_t* hinf);
// signature side of small packages: G2 membership (k_sig_subgroup's contract) and [r_i] sig_i
// (k_sig_scale's: mode selects the sets, r_i = 0 leaves a point unscaled)
hipError_t lsg_slp_g2_subgroup(hipStream_t st, int n, const uint32_t* sig_aff, const uint8_t* inf, int32_t* err);
hipError_t lsg_slp_g2_scale(hipStream_t st, int n, const uint32_t* sig_aff, const uint8_t* inf, const int32_t* err,
                            const uint8_t* pinf, const uint64_t* rnd, const uint8_t* mode, uint32_t* out);
// Miller items of one set each (lane-form P, pinf, hinf, err, H as for k_miller_fused):
// f[item] = ML(P_i, H_i) of set item_first[item], 1 for a set that does not take part
hipError_t lsg_slp_miller_items1(hipStream_t st, int n_items, const int32_t* item_first, const uint32_t* P,
                                 const uint8_t* pinf, const uint8_t* hinf, const int32_t* err, const uint32_t* H,
                                 uint32_t* f);
