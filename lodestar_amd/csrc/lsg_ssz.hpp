// lsg_ssz.hpp -- SHA-256's compression function and the SSZ signing roots built on it
// (computeSigningRoot, state-transition/src/util/signingRoot.ts:7-13):
// one text for the signing-root kernels of lsg_k_hash.hip and for tests/native/sszcheck.cpp,
// which runs it on the CPU, as lsg_bits.h is for the bitfield walk.  Plain integers only.
//
// The device build reaches this file through lsg_h2c.hpp with the backend's function macros
// in force; a plain host program includes it directly and gets inline functions.
#pragma once
#include <stdint.h>

#ifndef LSG_INL
#define LSG_INL inline
#endif
#ifndef LSG_BIGFN
#define LSG_BIGFN inline
#endif
#ifndef LSG_CONST
#define LSG_CONST static constexpr
#endif

// ------------------------------------------------------------------ SHA-256
LSG_CONST uint32_t SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

LSG_INL uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

LSG_BIGFN void sha256_compress(uint32_t* st, const uint32_t* blk) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = blk[i];
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      uint32_t s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
      uint32_t s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
      wi = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
      w[i & 15] = wi;
    }
    uint32_t S1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
    uint32_t ch = (e & f) ^ (~e & g);
    uint32_t t1 = h + S1 + ch + SHA_K[i] + wi;
    uint32_t S0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22);
    uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    uint32_t t2 = S0 + mj;
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
  st[5] += f;
  st[6] += g;
  st[7] += h;
}

LSG_INL void be_words_to_bytes(uint8_t* out, const uint32_t* w, int nw) {
  for (int i = 0; i < nw; i++) {
    out[4 * i] = (uint8_t)(w[i] >> 24);
    out[4 * i + 1] = (uint8_t)(w[i] >> 16);
    out[4 * i + 2] = (uint8_t)(w[i] >> 8);
    out[4 * i + 3] = (uint8_t)w[i];
  }
}

// ------------------------------------------------------------------ SSZ signing roots
// Chunks are 8 big-endian SHA-256 words; every node is SHA-256 of exactly 64 bytes, so its
// second block is the constant padding block of a 512-bit message.
LSG_INL void ssz_hash2(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                    0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t blk[16];
  for (int k = 0; k < 8; k++) {
    blk[k] = a[k];
    blk[8 + k] = b[k];
  }
  sha256_compress(st, blk);
  for (int k = 0; k < 16; k++) blk[k] = 0;
  blk[0] = 0x80000000u;
  blk[15] = 512;
  sha256_compress(st, blk);
  for (int k = 0; k < 8; k++) out[k] = st[k];
}

// `len` (<= 32) bytes at p as a zero-padded SSZ chunk (byte loads: p has no alignment)
LSG_INL void ssz_chunk(uint32_t* w, const uint8_t* p, int len) {
  for (int k = 0; k < 8; k++) {
    uint32_t v = 0;
    for (int j = 0; j < 4; j++) v = (v << 8) | (4 * k + j < len ? p[4 * k + j] : 0u);
    w[k] = v;
  }
}

LSG_INL void ssz_store(uint8_t* out, const uint32_t* w) { be_words_to_bytes(out, w, 8); }

// Every function below reads its whole object and its domain before it stores: `out` may be
// the object's own bytes (k_msg_roots writes a root over the start of its payload).

// hash_tree_root(SigningData{objectRoot, domain}) (util/signingRoot.ts:7-13): the object is
// its own root -- a Root, or (obj_len 8) a uint64 such as a Slot or an Epoch, whose root is
// its zero-padded chunk.  1 node hash.
LSG_INL void ssz_signing_root_chunk(const uint8_t* obj, int obj_len, const uint8_t* domain, uint8_t* out) {
  uint32_t r[8], d[8], o[8];
  ssz_chunk(r, obj, obj_len);
  ssz_chunk(d, domain, 32);
  ssz_hash2(r, d, o);
  ssz_store(out, o);
}

// a container of two uint64 fields (16 bytes: phase0.VoluntaryExit {epoch, validatorIndex},
// altair.SyncAggregatorSelectionData {slot, subcommitteeIndex}): 2 node hashes
LSG_INL void ssz_signing_root_u64x2(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], d[8];
  ssz_chunk(l0, a, 8);
  ssz_chunk(l1, a + 8, 8);
  ssz_chunk(d, domain, 32);
  ssz_hash2(l0, l1, l0);
  ssz_hash2(l0, d, l0);
  ssz_store(out, l0);
}

// capella.BLSToExecutionChange (76 bytes: validatorIndex u64, fromBlsPubkey Bytes48,
// toExecutionAddress Bytes20; signatureSets/blsToExecutionChange.ts): the key is two chunks
// under one node, 3 fields -> 4 leaves, 2 levels, then SigningData -- 5 node hashes
LSG_INL void ssz_signing_root_bls_change(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], t[8], z[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(l1, a + 8, 32);  // fromBlsPubkey
  ssz_chunk(t, a + 40, 16);
  ssz_hash2(l1, t, l1);
  ssz_chunk(l0, a, 8);  // validatorIndex
  ssz_hash2(l0, l1, l0);
  ssz_chunk(t, a + 56, 20);  // toExecutionAddress; leaf 3 is a zero chunk
  ssz_hash2(t, z, l1);
  ssz_hash2(l0, l1, t);  // BLSToExecutionChange.hashTreeRoot
  ssz_chunk(z, domain, 32);
  ssz_hash2(t, z, t);
  ssz_store(out, t);
}

// computeSigningRoot(ssz.phase0.DepositMessage, msg, domain) (block/processDeposit.ts:49-54)
// from the SSZ serialization of DepositMessage (88 bytes: pubkey 48, withdrawalCredentials 32,
// amount u64): the Bytes48 key is two chunks under one node, 3 fields -> 4 leaves, 2 levels,
// then SigningData -- 5 node hashes
LSG_INL void ssz_signing_root_deposit(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], t[8], z[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(l0, a, 32);  // pubkey
  ssz_chunk(t, a + 32, 16);
  ssz_hash2(l0, t, l0);
  ssz_chunk(l1, a + 48, 32);  // withdrawalCredentials
  ssz_hash2(l0, l1, l0);
  ssz_chunk(t, a + 80, 8);  // amount; leaf 3 is a zero chunk
  ssz_hash2(t, z, l1);
  ssz_hash2(l0, l1, t);  // DepositMessage.hashTreeRoot
  ssz_chunk(z, domain, 32);
  ssz_hash2(t, z, t);
  ssz_store(out, t);
}

// phase0.BeaconBlockHeader (112 bytes: slot u64, proposerIndex u64, parentRoot, stateRoot,
// bodyRoot; proposer slashings): 5 fields -> 8 leaves, 3 levels, then SigningData -- 8 node
// hashes
LSG_INL void ssz_signing_root_header(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8], z[8], z1[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(l0, a, 8);        // slot
  ssz_chunk(l1, a + 8, 8);    // proposerIndex
  ssz_chunk(l2, a + 16, 32);  // parentRoot
  ssz_chunk(l3, a + 48, 32);  // stateRoot
  ssz_chunk(l4, a + 80, 32);  // bodyRoot
  ssz_hash2(z, z, z1);        // leaves 5..7 are zero chunks
  ssz_hash2(l0, l1, l0);
  ssz_hash2(l2, l3, l2);
  ssz_hash2(l4, z, l4);
  ssz_hash2(l0, l2, l0);
  ssz_hash2(l4, z1, l4);
  ssz_hash2(l0, l4, l0);  // BeaconBlockHeader.hashTreeRoot
  ssz_chunk(z, domain, 32);
  ssz_hash2(l0, z, l0);
  ssz_store(out, l0);
}

// getAttestationDataSigningRoot (signatureSets/indexedAttestation.ts:11-19) from the SSZ
// serialization of phase0.AttestationData (128 bytes: slot u64, index u64, beaconBlockRoot,
// source {epoch u64, root}, target {epoch u64, root}): 5 fields -> 8 leaves, 3 levels, then
// SigningData -- 10 node hashes
LSG_INL void ssz_attestation_data_root(const uint8_t* a, uint32_t* t);
LSG_INL void ssz_signing_root_attestation(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t t[8], z[8];
  ssz_attestation_data_root(a, t);
  ssz_chunk(z, domain, 32);
  ssz_hash2(t, z, t);
  ssz_store(out, t);
}
// AttestationData.hashTreeRoot alone (the variable kinds hold one as a field): 9 node hashes
LSG_INL void ssz_attestation_data_root(const uint8_t* a, uint32_t* t) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8], z[8], z1[8], h01[8], h23[8], h45[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(l0, a, 8);        // slot
  ssz_chunk(l1, a + 8, 8);    // index
  ssz_chunk(l2, a + 16, 32);  // beaconBlockRoot
  ssz_chunk(t, a + 48, 8);    // source = Checkpoint{epoch, root}
  ssz_chunk(l3, a + 56, 32);
  ssz_hash2(t, l3, l3);
  ssz_chunk(t, a + 88, 8);  // target
  ssz_chunk(l4, a + 96, 32);
  ssz_hash2(t, l4, l4);
  ssz_hash2(z, z, z1);  // leaves 5..7 are zero chunks
  ssz_hash2(l0, l1, h01);
  ssz_hash2(l2, l3, h23);
  ssz_hash2(l4, z, h45);
  ssz_hash2(h01, h23, h01);
  ssz_hash2(h45, z1, h45);
  ssz_hash2(h01, h45, t);  // AttestationData.hashTreeRoot
}

// hash_tree_root of a 96-byte vector (a BLSSignature): 3 chunks -> 4 leaves, 3 node hashes
LSG_INL void ssz_root_bytes96(const uint8_t* p, uint32_t* out) {
  uint32_t a[8], b[8], z[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(a, p, 32);
  ssz_chunk(b, p + 32, 32);
  ssz_hash2(a, b, a);
  ssz_chunk(b, p + 64, 32);
  ssz_hash2(b, z, b);
  ssz_hash2(a, b, out);
}

// altair.ContributionAndProof (264 bytes: aggregatorIndex u64, contribution
// SyncCommitteeContribution {slot u64, beaconBlockRoot, subcommitteeIndex u64, aggregationBits
// Bitvector[128], signature}, selectionProof; altair/sszTypes.ts:57-75;
// signatureSets/contributionAndProof.ts): the contribution is 5 fields -> 8 leaves, the object
// 3 fields -> 4 leaves, then SigningData -- 17 node hashes
LSG_INL void ssz_signing_root_contribution_and_proof(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8], t[8], z[8], z1[8];
  for (int k = 0; k < 8; k++) z[k] = 0;
  ssz_chunk(l0, a + 8, 8);    // contribution.slot
  ssz_chunk(l1, a + 16, 32);  // beaconBlockRoot
  ssz_chunk(l2, a + 48, 8);   // subcommitteeIndex
  ssz_chunk(l3, a + 56, 16);  // aggregationBits
  ssz_root_bytes96(a + 72, l4);  // signature
  ssz_hash2(z, z, z1);        // leaves 5..7 are zero chunks
  ssz_hash2(l0, l1, l0);
  ssz_hash2(l2, l3, l2);
  ssz_hash2(l4, z, l4);
  ssz_hash2(l0, l2, l0);
  ssz_hash2(l4, z1, l4);
  ssz_hash2(l0, l4, l0);  // SyncCommitteeContribution.hashTreeRoot
  ssz_chunk(t, a, 8);     // aggregatorIndex
  ssz_hash2(t, l0, l0);
  ssz_root_bytes96(a + 168, t);  // selectionProof; leaf 3 is a zero chunk
  ssz_hash2(t, z, t);
  ssz_hash2(l0, t, t);  // ContributionAndProof.hashTreeRoot
  ssz_chunk(z, domain, 32);
  ssz_hash2(t, z, t);
  ssz_store(out, t);
}

// computeSigningRoot of the object kind that an SSZ serialization of obj_len bytes selects
// (include/lodestar_bls.h, LSG_MSG_OBJECT: every kind has its own length); false, and nothing
// stored, for a length that names no kind
LSG_INL bool ssz_object_signing_root(uint32_t obj_len, const uint8_t* obj, const uint8_t* domain, uint8_t* out) {
  switch (obj_len) {
    case 8:
    case 32: ssz_signing_root_chunk(obj, (int)obj_len, domain, out); return true;
    case 16: ssz_signing_root_u64x2(obj, domain, out); return true;
    case 76: ssz_signing_root_bls_change(obj, domain, out); return true;
    case 88: ssz_signing_root_deposit(obj, domain, out); return true;
    case 112: ssz_signing_root_header(obj, domain, out); return true;
    case 128: ssz_signing_root_attestation(obj, domain, out); return true;
    case 264: ssz_signing_root_contribution_and_proof(obj, domain, out); return true;
    default: return false;
  }
}

// ------------------------------------------------------------------ variable-size kinds
// phase0.AggregateAndProof (kind 1; phase0/sszTypes.ts:460, Attestation :319, Bitlist[2048]) and
// EIP-7549's AggregateAndProof (kind 2; consensus-specs electra: Attestation {aggregation_bits:
// Bitlist[131072], data, signature, committee_bits: Bitvector[64]}), serialized as
//   [0,8) aggregatorIndex  [8,12) offset 108  [12,108) selectionProof  [108,112) inner offset
//   [112,240) AttestationData  [240,336) signature  [336,344) committee_bits (kind 2)
//   then the bitlist with its delimiter bit.
//   bits_root        = H(merkleize(pack_bits(bits), limit_chunks), le256(n))   limit 8 / 512 chunks
//   attestation_root = merkle root of [bits_root, data_root, htr(signature), 0 / committee_bits]
//   object_root      = merkle root of [aggregatorIndex, attestation_root, htr(selectionProof), 0]
// One object is hashed by 64 lanes in phases with a barrier after each; ssz_var_step is what
// lane `lane` does in phase `phase`.  k_msg_roots_var runs it with one workgroup per object and
// __syncthreads() between phases; tests/native/sszvarcheck.cpp steps 64 logical lanes phase by
// phase.  A phase reads only the payload and nodes that earlier phases stored, so both orders
// of execution compute the same.  The structure is assumed valid (lsgp::msg_var_ok).
//
// Zero-subtree hashes: SSZ_ZERO[d] is the root of a depth-d tree of zero chunks.  A level with
// an odd number of nodes pairs its last node with SSZ_ZERO[level]; padding is never hashed.
LSG_CONST uint32_t SSZ_ZERO[10][8] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xf5a5fd42u, 0xd16a2030u, 0x2798ef6eu, 0xd309979bu, 0x43003d23u, 0x20d9f0e8u, 0xea9831a9u, 0x2759fb4bu},
    {0xdb56114eu, 0x00fdd4c1u, 0xf85c892bu, 0xf35ac9a8u, 0x9289aaecu, 0xb1ebd0a9u, 0x6cde606au, 0x748b5d71u},
    {0xc78009fdu, 0xf07fc56au, 0x11f12237u, 0x0658a353u, 0xaaa542edu, 0x63e44c4bu, 0xc15ff4cdu, 0x105ab33cu},
    {0x536d9883u, 0x7f2dd165u, 0xa55d5eeau, 0xe9148595u, 0x4472d56fu, 0x246df256u, 0xbf3cae19u, 0x352a123cu},
    {0x9efde052u, 0xaa15429fu, 0xae05bad4u, 0xd0b1d7c6u, 0x4da64d03u, 0xd7a1854au, 0x588c2cb8u, 0x430c0d30u},
    {0xd88ddfeeu, 0xd400a875u, 0x5596b219u, 0x42c1497eu, 0x114c302eu, 0x6118290fu, 0x91e67729u, 0x76041fa1u},
    {0x87eb0ddbu, 0xa57e35f6u, 0xd2866738u, 0x02a4af59u, 0x75e22506u, 0xc7cf4c64u, 0xbb6be5eeu, 0x11527f2cu},
    {0x26846476u, 0xfd5fc54au, 0x5d433851u, 0x67c95144u, 0xf2643f53u, 0x3cc85bb9u, 0xd16b782fu, 0x8d7db193u},
    {0x506d8658u, 0x2d252405u, 0xb8400187u, 0x92cad2bfu, 0x1259f1efu, 0x5aa5f887u, 0xe13cb2f0u, 0x094f51e1u}};

#define SSZ_VAR_LANES 64
// Node storage (LDS on the device): tree levels alternate between buffer A (256 nodes: levels
// 1, 3, ...) and buffer B (128 nodes: levels 2, 4, ...), so a phase never stores where a lane
// of the same phase reads; word k of node j is at k * capacity + j (neighbouring lanes,
// neighbouring words).  Three more nodes hold the fixed part's subtree roots.  12,384 bytes.
#define SSZ_VAR_NODE_WORDS ((256 + 128 + 3) * 8)
#define SSZ_VAR_FIX_DATA 0  // AttestationData root
#define SSZ_VAR_FIX_SIG 1   // H(htr(signature), committee_bits chunk or 0)
#define SSZ_VAR_FIX_SEL 2   // H(htr(selectionProof), 0)
#define SSZ_VAR_LANE_DATA 63
#define SSZ_VAR_LANE_SIG 62
#define SSZ_VAR_LANE_SEL 61

struct SszVar {
  uint32_t bits_off;  // where the bitlist starts: 336 / 344
  uint32_t bits_len;  // its bytes, delimiter included
  uint32_t n_bits;
  uint32_t chunks;  // 32-byte chunks of pack_bits (0 for an empty list)
  uint32_t depth;   // of the chunk tree: 3 (8 chunks) / 9 (512 chunks)
  uint32_t levels;  // tree levels that hold more than one node: the phases before the last
  bool electra;
};
LSG_INL uint32_t ssz_var_bits_off(uint32_t kind) { return kind == 2 ? 344u : 336u; }
LSG_INL uint32_t ssz_var_max_bits(uint32_t kind) { return kind == 2 ? 131072u : 2048u; }
// `last`: the object's last byte (the bitlist's, which holds the delimiter bit)
LSG_INL SszVar ssz_var_shape(uint32_t kind, uint32_t obj_len, uint8_t last) {
  SszVar v;
  v.electra = kind == 2;
  v.bits_off = ssz_var_bits_off(kind);
  v.bits_len = obj_len - v.bits_off;
  uint32_t top = 0;
  while (top < 7 && (last >> (top + 1))) top++;
  v.n_bits = 8 * (v.bits_len - 1) + top;
  v.chunks = (v.n_bits + 255) / 256;
  v.depth = v.electra ? 9 : 3;
  v.levels = 0;
  while (((v.chunks + (1u << v.levels) - 1) >> v.levels) > 1) v.levels++;
  return v;
}
// nodes of tree level l (level 0: the chunks; an empty list is one zero chunk)
LSG_INL uint32_t ssz_var_level_count(const SszVar& v, uint32_t l) {
  const uint32_t c0 = v.chunks ? v.chunks : 1;
  return (c0 + (1u << l) - 1) >> l;
}
// barrier-separated phases: one per tree level with more than one node (at least one: phase 0
// also hashes the fixed part), then lane 0's last one
LSG_INL uint32_t ssz_var_phases(const SszVar& v) { return (v.levels ? v.levels : 1) + 1; }
LSG_INL uint32_t ssz_var_node_at(uint32_t level, uint32_t j, uint32_t k) {
  return (level & 1) ? k * 256 + j : 2048 + k * 128 + j;
}
LSG_INL uint32_t ssz_var_fix_at(uint32_t f, uint32_t k) { return (256 + 128) * 8 + 8 * f + k; }
// A node by value, and the one node hash the variable kinds call.  The device build makes it a
// real call (LSG_SSZ_CALL, set by lsg_h2c.hpp): the phases below hash at some thirty places,
// and the compression function inlined at each made a kernel of several hundred thousand
// instructions.  Operands and result travel in registers.
#ifndef LSG_SSZ_CALL
#define LSG_SSZ_CALL inline
#define LSG_SSZ_CALL_DEFAULTED 1  // (lsg_h2c.hpp refuses a device build that got here first)
#endif
struct SszNode {
  uint32_t w[8];
};
LSG_SSZ_CALL SszNode ssz_node_hash(SszNode a, SszNode b) {
  SszNode o;
  ssz_hash2(a.w, b.w, o.w);
  return o;
}
LSG_INL SszNode ssz_node_chunk(const uint8_t* p, int len) {
  SszNode n;
  ssz_chunk(n.w, p, len);
  return n;
}
LSG_INL SszNode ssz_node_zero(uint32_t depth) {
  SszNode n;
  for (uint32_t k = 0; k < 8; k++) n.w[k] = SSZ_ZERO[depth][k];
  return n;
}
// hash_tree_root of a 96-byte vector, as ssz_root_bytes96
LSG_INL SszNode ssz_node_bytes96(const uint8_t* p) {
  const SszNode lo = ssz_node_hash(ssz_node_chunk(p, 32), ssz_node_chunk(p + 32, 32));
  return ssz_node_hash(lo, ssz_node_hash(ssz_node_chunk(p + 64, 32), ssz_node_zero(0)));
}
// AttestationData.hashTreeRoot, as ssz_attestation_data_root: 9 node hashes
LSG_INL SszNode ssz_node_attestation_data(const uint8_t* a) {
  const SszNode src = ssz_node_hash(ssz_node_chunk(a + 48, 8), ssz_node_chunk(a + 56, 32));
  const SszNode tgt = ssz_node_hash(ssz_node_chunk(a + 88, 8), ssz_node_chunk(a + 96, 32));
  const SszNode h01 = ssz_node_hash(ssz_node_chunk(a, 8), ssz_node_chunk(a + 8, 8));
  const SszNode h23 = ssz_node_hash(ssz_node_chunk(a + 16, 32), src);
  const SszNode h45 = ssz_node_hash(tgt, ssz_node_zero(0));
  const SszNode lo = ssz_node_hash(h01, h23);
  return ssz_node_hash(lo, ssz_node_hash(h45, ssz_node_hash(ssz_node_zero(0), ssz_node_zero(0))));
}

// chunk c of pack_bits: the bitlist's bytes without the delimiter bit, zero-padded
LSG_INL SszNode ssz_var_bits_chunk(const SszVar& v, const uint8_t* bits, uint32_t c) {
  const uint32_t nbytes = (v.n_bits + 7) / 8;
  SszNode n;
  for (uint32_t k = 0; k < 8; k++) {
    uint32_t x = 0;
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t at = 32 * c + 4 * k + j;
      uint32_t b = at < nbytes ? bits[at] : 0u;
      if (at == v.bits_len - 1) b &= (1u << (v.n_bits & 7)) - 1;  // the delimiter bit
      x = (x << 8) | b;
    }
    n.w[k] = x;
  }
  return n;
}
// node j of level l: a chunk of the payload, or a stored node
LSG_INL SszNode ssz_var_load(const SszVar& v, const uint8_t* obj, const uint32_t* nodes, uint32_t l, uint32_t j) {
  if (l == 0) return ssz_var_bits_chunk(v, obj + v.bits_off, j);
  SszNode n;
  for (uint32_t k = 0; k < 8; k++) n.w[k] = nodes[ssz_var_node_at(l, j, k)];
  return n;
}
LSG_INL SszNode ssz_var_fix_load(const uint32_t* nodes, uint32_t f) {
  SszNode n;
  for (uint32_t k = 0; k < 8; k++) n.w[k] = nodes[ssz_var_fix_at(f, k)];
  return n;
}

// What lane `lane` (0..63) does in phase `phase` (0..ssz_var_phases - 1); returns the node
// hashes it ran, one after the other.  `out` (32 bytes, written by lane 0 in the last phase,
// after everything is read) may be the start of obj.
//   phase p < levels   round r: lane hashes pair 64 r + lane of level p into level p + 1
//   phase 0            lanes 63, 62, 61 also hash the AttestationData, signature and
//                      selection-proof subtrees (9, 4, 4 hashes)
//   last phase         lane 0: the remaining levels against zero hashes, the length mix-in,
//                      the two containers and SigningData (depth - levels + 6 hashes)
// Over the phases the busiest lanes run at most sum over levels of ceil(pairs / 64), plus 15.
LSG_INL uint32_t ssz_var_step(const SszVar& v, uint32_t phase, uint32_t lane, const uint8_t* obj, const uint8_t* domain,
                              uint32_t* nodes, uint8_t* out) {
  uint32_t nh = 0;
  if (phase + 1 < ssz_var_phases(v)) {
    if (phase < v.levels) {
      const uint32_t cnt = ssz_var_level_count(v, phase), pairs = (cnt + 1) >> 1;
      for (uint32_t j = lane; j < pairs; j += SSZ_VAR_LANES) {
        const SszNode a = ssz_var_load(v, obj, nodes, phase, 2 * j);
        const SszNode b = 2 * j + 1 < cnt ? ssz_var_load(v, obj, nodes, phase, 2 * j + 1) : ssz_node_zero(phase);
        const SszNode h = ssz_node_hash(a, b);
        for (uint32_t k = 0; k < 8; k++) nodes[ssz_var_node_at(phase + 1, j, k)] = h.w[k];
        nh++;
      }
    }
    if (phase == 0 && lane >= SSZ_VAR_LANE_SEL) {
      uint32_t f;
      SszNode h;
      if (lane == SSZ_VAR_LANE_DATA) {
        f = SSZ_VAR_FIX_DATA;
        h = ssz_node_attestation_data(obj + 112);
        nh += 9;
      } else {
        const bool sig = lane == SSZ_VAR_LANE_SIG;
        f = sig ? SSZ_VAR_FIX_SIG : SSZ_VAR_FIX_SEL;
        // beside the signature: Electra's committee_bits chunk; else a zero chunk
        h = ssz_node_hash(ssz_node_bytes96(obj + (sig ? 240 : 12)), ssz_node_chunk(obj + 336, sig && v.electra ? 8 : 0));
        nh += 4;
      }
      for (uint32_t k = 0; k < 8; k++) nodes[ssz_var_fix_at(f, k)] = h.w[k];
    }
    return nh;
  }
  if (lane != 0) return 0;
  SszNode a = ssz_var_load(v, obj, nodes, v.levels, 0);
  for (uint32_t l = v.levels; l < v.depth; l++) a = ssz_node_hash(a, ssz_node_zero(l));
  SszNode len = ssz_node_zero(0);  // le256(n_bits) as big-endian words
  len.w[0] = ((v.n_bits & 0xffu) << 24) | ((v.n_bits & 0xff00u) << 8) | ((v.n_bits >> 8) & 0xff00u) | (v.n_bits >> 24);
  a = ssz_node_hash(a, len);  // mix_in_length: bits_root
  a = ssz_node_hash(a, ssz_var_fix_load(nodes, SSZ_VAR_FIX_DATA));
  a = ssz_node_hash(a, ssz_var_fix_load(nodes, SSZ_VAR_FIX_SIG));  // Attestation.hashTreeRoot
  a = ssz_node_hash(ssz_node_chunk(obj, 8), a);                    // aggregatorIndex beside it
  a = ssz_node_hash(a, ssz_var_fix_load(nodes, SSZ_VAR_FIX_SEL));  // AggregateAndProof.hashTreeRoot
  a = ssz_node_hash(a, ssz_node_chunk(domain, 32));
  ssz_store(out, a.w);
  return v.depth - v.levels + 6;
}
