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
LSG_INL void ssz_signing_root_attestation(const uint8_t* a, const uint8_t* domain, uint8_t* out) {
  uint32_t l0[8], l1[8], l2[8], l3[8], l4[8], t[8], z[8], z1[8], h01[8], h23[8], h45[8];
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
    default: return false;
  }
}
