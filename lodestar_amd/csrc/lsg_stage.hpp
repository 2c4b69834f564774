// lsg_stage.hpp -- host-only staging of a package: how the caller's sets (untrusted pointers,
// lengths and blobs) become the bytes the kernels read.  The layout of the pinned staging arena
// (StageLayout, the one statement of its size), the table that finds the distinct messages
// (msg_key, MsgTable, sample_repeats), a measuring pass (stage_measure: what the buffers must
// hold, before anything is written), a filling pass (stage_fill: signatures, messages through
// the message cache, key slots, committee bit fields, plan words) and the RLC randomizers
// (draw_randomizers).  Bytes and small integers: no device, no environment, no Slot -- the
// key function and the entropy source are parameters.  lsg_host.hip's stage_sets sizes its
// buffers between the two passes and issues the copies; tests/native/stagecheck.cpp drives
// both passes on the CPU over allocations of exactly the promised sizes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lsg_msg_cache.hpp"
#include "lsg_plan.hpp"

namespace lsgp {

inline uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// ---- the pinned staging arena of up to n sets / npk keys of `stride` bytes / mb message bytes:
// byte offsets of its nine fields (each 8-aligned, in this order, at least one entry each)
// and its size, the end of the last.  Per set: 192 signature bytes, the signature length, its message's offset,
// length word and id, the randomizer; per key: its length and its slot.
struct StageLayout {
  size_t sig = 0, siglen = 0, msgoff = 0, msglen = 0, mid = 0, pklen = 0, rnd = 0, pk = 0, msg = 0;
  size_t bytes = 0;
  size_t nn = 1, np = 1, stride = 96, mb = 1;  // the counts the offsets were made for (floored at 1)
};
inline StageLayout stage_layout(size_t n, size_t npk, size_t stride, size_t msg_bytes) {
  auto al = [](size_t x) { return (x + 7) & ~(size_t)7; };
  StageLayout L;
  L.nn = std::max(n, (size_t)1);
  L.np = std::max(npk, (size_t)1);
  L.stride = stride;
  L.mb = std::max(msg_bytes, (size_t)1);
  L.sig = 0;
  L.siglen = al(L.sig + 192 * L.nn);
  L.msgoff = al(L.siglen + 4 * L.nn);
  L.msglen = al(L.msgoff + 4 * L.nn);
  L.mid = al(L.msglen + 4 * L.nn);
  L.pklen = al(L.mid + 4 * L.nn);
  L.rnd = al(L.pklen + 4 * L.np);
  L.pk = al(L.rnd + 8 * L.nn);
  L.msg = al(L.pk + stride * L.np);
  L.bytes = L.msg + L.mb;
  return L;
}

// ---- distinct messages
// 64-bit mix of a message (its length and 8-byte words; signing roots are SHA-256 outputs).
// msg_len as the set carries it: an LSG_MSG_OBJECT marker goes into the mix, not the byte count
inline uint64_t msg_key(const uint8_t* m, uint32_t msg_len) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ msg_len;
  const uint32_t len = msg_bytes(msg_len);
  uint32_t k = 0;
  for (; k + 8 <= len; k += 8) {
    uint64_t w;
    memcpy(&w, m + k, 8);
    h = (h ^ w) * 0xff51afd7ed558ccdull;
    h ^= h >> 32;
  }
  for (; k < len; k++) h = (h ^ m[k]) * 0x100000001b3ull;
  return h ^ (h >> 29);
}
struct MsgKey {
  uint64_t operator()(const lsg_set& t) const { return msg_key(t.msg, t.msg_len); }
};

// Open-addressing table over the messages of one package: slot -> distinct message id (first:
// the set that brought it), with the message's 64-bit key beside it so that a probe compares
// bytes only on a key match.  The caller keeps one and reuses its storage from package to package.
struct MsgTable {
  std::vector<uint32_t> tab, first;
  std::vector<uint64_t> key;
  size_t cap = 0;  // 0: no table for this package (every set's message counts as new)

  void begin(size_t n) {
    cap = 16;
    while (cap < 2 * n) cap <<= 1;
    tab.assign(cap, UINT32_MAX);
    key.resize(cap);
    first.resize(n);
  }
  // the id of set i's message (key k): an earlier one with the same length word and bytes, or
  // `next`, which set i then owns
  uint32_t find_or_add(const lsg_set* const* sets, size_t i, uint64_t k, uint32_t next) {
    const lsg_set* q = sets[i];
    for (size_t h = (size_t)k & (cap - 1);; h = (h + 1) & (cap - 1)) {
      const uint32_t e = tab[h];
      if (e == UINT32_MAX) {
        tab[h] = next;
        key[h] = k;
        first[next] = (uint32_t)i;
        return next;
      }
      if (key[h] != k) continue;
      const lsg_set* r = sets[first[e]];
      if (r->msg_len == q->msg_len && (q->msg_len == 0 || memcmp(r->msg, q->msg, msg_bytes(q->msg_len)) == 0)) return e;
    }
  }
};

// A package whose sample of 256 evenly spaced sets shows no repeated key is taken as all
// distinct and staged without the table (the firehose of distinct gossip messages pays ~5 us,
// not the table's ~1 ms under the context lock); committee-shaped packages repeat at once.
template <class KeyFn>
inline bool sample_repeats(const lsg_set* const* sets, size_t n, KeyFn&& key_of) {
  const size_t k = std::min(n, (size_t)256), step = n / k;
  uint64_t seen[512];
  bool used[512] = {false};
  for (size_t j = 0; j < k; j++) {
    const uint64_t key = key_of(*sets[j * step]);
    for (size_t h = (size_t)key & 511;; h = (h + 1) & 511) {
      if (!used[h]) {
        used[h] = true;
        seen[h] = key;
        break;
      }
      if (seen[h] == key) return true;
    }
  }
  return false;
}

// ---- the measuring pass: what staging these sets will need, read from their counts and
// length words alone (and a multi set's leading count word).
// bits_ok: a set with pk_len == LSG_PK_BITS names its keys by committee id + participation bits,
// one with LSG_PK_BITS_MULTI by a committee list + one bitfield (the entry points that take
// sets); false where the caller passes one key list of one length (lsg_aggregate_pubkeys, the
// table and KeyValidate calls), which keeps treating both as unknown key lengths.
struct StageSizes {
  size_t npk = 0;        // key slots (sets given by bits have none)
  size_t msg_total = 0;  // message bytes of every set, repeats included
  size_t n_bits_sets = 0, n_multi = 0;
  size_t bit_words = 0;  // words of the bit arena the bits and multi sets may take
  bool all_index = true;  // every key names a table row: 4-byte key slots (a block body's
                          // ~3.7M signers cross PCIe as 15 MB instead of 355 MB)
  bool any_obj = false;   // a message is an SSZ object + domain (LSG_MSG_OBJECT, tag 0): k_msg_roots runs
  bool any_var = false;   // a message is a tagged, variable-size object: k_msg_roots_var runs
  size_t pk_stride() const { return all_index ? 4 : 96; }
};
inline bool stage_is_bits(const lsg_set& t, bool bits_ok) { return bits_ok && t.pk_len == LSG_PK_BITS; }
// (the entry points have refused a multi set without a blob or with more than
// LSG_MAX_SET_COMMITTEES ids; one that comes through all the same is a bad committee)
inline bool stage_is_multi(const lsg_set& t, bool bits_ok) { return bits_ok && t.pk_len == LSG_PK_BITS_MULTI; }
inline StageSizes stage_measure(const lsg_set* const* sets, size_t n, bool bits_ok) {
  StageSizes z;
  for (size_t i = 0; i < n; i++) {
    const lsg_set& t = *sets[i];
    z.msg_total += msg_bytes(t.msg_len);
    z.any_obj = z.any_obj || msg_fixed_object(t.msg_len);
    z.any_var = z.any_var || msg_kind_tag(t.msg_len) != 0;
    if (stage_is_bits(t, bits_ok)) {
      z.n_bits_sets++;
      z.bit_words += bits_words(t.n_pks);
    } else if (stage_is_multi(t, bits_ok)) {  // every part on its own word: up to k words more
      z.n_multi++;
      z.bit_words += bits_words(t.n_pks) + (multi_set_ok(t) ? multi_k(t) : 0);
    } else {
      z.npk += t.n_pks;
      if (t.n_pks && t.pk_len != LSG_PK_INDEX) z.all_index = false;
    }
  }
  return z;
}

// ---- the RLC randomizers of n sets into rnd: the caller's (rnd_in, each nonzero, checked at
// the entry point), a splitmix64 stream from `seed` with zeros skipped (tests), or -- seed 0 --
// from `entropy(buf, len)` with zeros redrawn; false from it is LSG_ERR_ENTROPY, and there is no
// deterministic fallback: predictable multipliers would let forged sets cancel.  Sets that form
// a group of their own are verified as they are (maybeBatch.ts:34-38: one set is a plain
// verify): noscale[i] sets r_i = 0, which means "not scaled" to k_pk_scale and k_sig_scale.
// !scale: every r_i = 0.
template <class Entropy>
inline int draw_randomizers(uint64_t* rnd, size_t n, bool scale, const uint64_t* rnd_in, uint64_t seed,
                            const std::vector<uint8_t>* noscale, Entropy&& entropy) {
  if (!n) return LSG_OK;
  if (!scale) {
    memset(rnd, 0, 8 * n);
    return LSG_OK;
  }
  if (rnd_in) {
    memcpy(rnd, rnd_in, 8 * n);
  } else if (seed == 0) {
    if (!entropy((void*)rnd, 8 * n)) return LSG_ERR_ENTROPY;
    for (size_t i = 0; i < n; i++)
      while (rnd[i] == 0)
        if (!entropy((void*)&rnd[i], (size_t)8)) return LSG_ERR_ENTROPY;
  } else {
    uint64_t sd = seed;
    for (size_t i = 0; i < n; i++) {
      uint64_t r;
      do r = splitmix64(sd);
      while (r == 0);
      rnd[i] = r;
    }
  }
  if (noscale)
    for (size_t i = 0; i < n; i++)
      if ((*noscale)[i]) rnd[i] = 0;
  return LSG_OK;
}

// ---- the filling pass
// a message-cache source word that names an arena row (lsg_launch.h's LSG_MC_ROW, which the
// kernels read: lsg_host.hip asserts the two equal)
constexpr uint32_t MC_ROW = 0x80000000u;

struct StageOpts {
  bool scale = false;                            // draw randomizers (else all zero)
  const std::vector<uint8_t>* noscale = nullptr;  // per set: leave it unscaled
  bool dedup = false;      // stage each distinct message once
  bool dedup_on = true;    // the LSG_MSG_DEDUP switch (false: never, whatever `dedup` asks)
  bool bits_ok = false;    // as for stage_measure
  const uint64_t* rnd_in = nullptr;  // the caller's randomizers, one per set, in place of the draws
  uint64_t seed = 0;
};
// the registered committees, read-only: per id its length and whether it is set
struct Committees {
  const uint32_t* len = nullptr;
  const uint8_t* ok = nullptr;
  size_t count = 0;
  bool has(uint32_t id) const { return id < count && ok[id]; }
};

// What staging a package leaves behind on the host (lsg_host.hip's Slot is one of these; the
// vectors keep their storage from package to package).
struct Staged {
  size_t n_sets = 0, n_pks = 0;
  uint32_t pk_stride = 96;   // bytes per key slot: 4 when every key is a table index
  std::vector<uint64_t> rnd;
  // distinct messages of the staged package: set i hashes message msg_id[i] (n_msgs of them);
  // msg_dedup when some sets share one (a committee's attestations sign one AttestationData)
  size_t n_msgs = 0;
  bool msg_dedup = false;
  bool msg_objs = false;  // a staged message is an SSZ object + domain (LSG_MSG_OBJECT, tag 0)
  bool msg_vars = false;  // a staged message is a tagged, variable-size object
  std::vector<uint32_t> msg_id;  // host copy of the set -> message map (msg_dedup)
  size_t msg_used = 0;           // message bytes staged (each distinct message / miss once)
  // the message cache.  mc_on: the package was staged through it -- n_miss of the
  // n_msgs distinct messages are staged and hashed, mc_hits come from arena rows (mc_pins:
  // pinned until the launch's completion is observed), mc_pend rows are written by
  // k_h2c_cache_store and published then.  Plan arena: one source word per distinct message at
  // mc_src_off (MC_ROW | row, or the miss index), the (miss, row) pairs of the store
  // (mc_store) at mc_st_off.
  bool mc_on = false;
  uint64_t mc_epoch = 0;
  size_t n_miss = 0, mc_hits = 0, mc_src_off = 0, mc_st_off = 0;
  std::vector<uint32_t> mc_pins, mc_pend;
  std::vector<int32_t> mc_store;
  bool single_keys = false;  // every set has exactly one key (key i is set i's)
  // sets given as committee id + participation bits (LSG_PK_BITS) and as a
  // committee list + one bitfield (LSG_PK_BITS_MULTI), their fields in the bit arena (bit_words
  // of it in use); pk_all_bits: no other kind of set.  A multi set is a bits set to everything
  // else (shape.bits_p / bits_kerr).
  std::vector<BitsSet> bits_sets;
  std::vector<MultiSet> multi_sets;
  std::vector<MultiPart> multi_parts;
  bool pk_all_bits = false;
  size_t bit_words = 0;
  // the package's shape: the stager fills its per-set fields (pk_cnt, pk_first, bits_p,
  // bits_kerr), shape_jobs the rest
  PkgShape shape;
};

// Stages sets[0..n) (z: their stage_measure) into the arena A laid out by L (made for at least
// n sets, z.npk keys of z.pk_stride() bytes and z.msg_total message bytes) and the bit arena
// cbits (at least z.bit_words words; unused without bits and multi sets).  A bits or multi set
// stages its id(s) and bits only -- no key slots, no per-key error entries -- and its
// set-level errors are resolved here: an unknown or unset committee or a length mismatch
// (LSG_ERR_BAD_COMMITTEE, shape.bits_kerr), no participant (shape.bits_p 0).
// mc: the message cache or null; used when the package dedups, and then every distinct message
// is looked up, so the table is always built -- the sample would hide messages that repeat
// across packages.  Its source words and store pairs are appended to `plan`.
// Returns LSG_OK, or LSG_ERR_ENTROPY from draw_randomizers (out.rnd is not written then).
template <class KeyFn, class Entropy>
inline int stage_fill(uint8_t* A, const StageLayout& L, uint32_t* cbits, const lsg_set* const* sets, size_t n,
                      const StageSizes& z, const StageOpts& o, MsgCache* mc, const Committees& cm, MsgTable& mt,
                      std::vector<int32_t>& plan, Staged& out, KeyFn&& key_of, Entropy&& entropy) {
  const size_t n_by_bits = z.n_bits_sets + z.n_multi;
  const bool all_index = z.all_index;
  out.n_sets = n;
  out.n_pks = z.npk;
  out.pk_stride = (uint32_t)z.pk_stride();
  out.bits_sets.clear();
  out.multi_sets.clear();
  out.multi_parts.clear();
  out.shape.bits_p.clear();
  out.shape.bits_kerr.clear();
  out.pk_all_bits = n > 0 && n_by_bits == n;
  if (n_by_bits) {
    out.shape.bits_p.assign(n, -1);
    out.shape.bits_kerr.assign(n, 0);
    out.bits_sets.reserve(z.n_bits_sets);
    out.multi_sets.reserve(z.n_multi);
  }
  size_t bw = 0;  // words of the bit arena in use
  uint32_t* siglen = (uint32_t*)(A + L.siglen);
  uint32_t* msgoff = (uint32_t*)(A + L.msgoff);
  uint32_t* msglen = (uint32_t*)(A + L.msglen);
  uint32_t* mid = (uint32_t*)(A + L.mid);
  uint32_t* pklen = (uint32_t*)(A + L.pklen);
  uint64_t* rnd = (uint64_t*)(A + L.rnd);
  siglen[0] = msgoff[0] = msglen[0] = pklen[0] = 0;
  rnd[0] = 0;
  out.shape.pk_cnt.resize(n);
  out.shape.pk_first.resize(n);
  out.rnd.resize(n);
  size_t mo = 0, po = 0, nm = 0;
  bool single = z.npk == n && n_by_bits == 0;
  const bool dedup = o.dedup && o.dedup_on;
  if (!(dedup && mc && mc->capacity())) mc = nullptr;
  out.mc_on = mc != nullptr;
  out.n_miss = out.mc_hits = 0;
  out.mc_pins.clear();
  out.mc_pend.clear();
  out.mc_store.clear();
  bool miss_obj = false, miss_var = false;
  if (mc) {
    out.mc_epoch = mc->epoch();
    out.mc_src_off = plan.size();
    plan.resize(out.mc_src_off + n);
  }
  mt.cap = 0;
  if (dedup && n > 0 && (mc || (n > 1 && sample_repeats(sets, n, key_of)))) mt.begin(n);
  for (size_t i = 0; i < n; i++) {
    const lsg_set* q = sets[i];
    siglen[i] = q->sig_len;
    uint8_t* sg = A + L.sig + 192 * i;
    if ((q->sig_len == 96 || q->sig_len == 192) && q->sig)
      memcpy(sg, q->sig, q->sig_len);
    else
      memset(sg, 0, 96);
    uint64_t key = 0;
    uint32_t id = (uint32_t)nm;
    if (mt.cap) {
      key = key_of(*q);
      id = mt.find_or_add(sets, i, key, id);
    }
    mid[i] = id;
    if (id == nm) {  // a new message: staged once -- through the cache from its row, or as a miss
      const uint32_t mb = msg_bytes(q->msg_len);
      size_t k = nm;  // its staged entry
      bool staged = true;
      if (mc) {
        uint32_t row = 0;
        bool hit = false, store = false;
        if (!MsgCache::cacheable(mb) || !q->msg) {
          mc->note_bypass();
        } else {
          const MsgCache::Result r = mc->lookup(key, q->msg, q->msg_len, mb, &row);
          hit = r == MsgCache::HIT;
          store = r == MsgCache::MISS && mc->allot(key, q->msg, q->msg_len, mb, &row);
        }
        if (hit) {
          out.mc_pins.push_back(row);
          out.mc_hits++;
          plan[out.mc_src_off + nm] = (int32_t)(MC_ROW | row);
          staged = false;
        } else {
          k = out.n_miss++;
          if (store) {
            out.mc_pend.push_back(row);
            out.mc_store.push_back((int32_t)k);
            out.mc_store.push_back((int32_t)row);
          }
          plan[out.mc_src_off + nm] = (int32_t)k;
          miss_obj = miss_obj || msg_fixed_object(q->msg_len);
          miss_var = miss_var || msg_kind_tag(q->msg_len) != 0;
        }
      }
      if (staged) {
        msgoff[k] = (uint32_t)mo;
        msglen[k] = q->msg_len;  // (with its marker and tag: k_msg_roots / k_msg_roots_var turn the payload into a 32-byte message)
        if (mb) memcpy(A + L.msg + mo, q->msg, mb);
        mo += mb;
      }
      nm++;
    }
    out.shape.pk_first[i] = (uint32_t)po;
    if (stage_is_bits(*q, o.bits_ok)) {
      out.shape.pk_cnt[i] = 0;
      BitsSet b;
      b.out = (int32_t)i;
      uint32_t cid = 0;
      if (q->pks) memcpy(&cid, q->pks, 4);
      if (!q->pks || !cm.has(cid) || cm.len[cid] != q->n_pks)
        out.shape.bits_kerr[i] = LSG_ERR_BAD_COMMITTEE;
      else
        b = bits_stage_set(cid, q->pks + 4, q->n_pks, (int32_t)i, cbits, &bw);
      out.shape.bits_p[i] = (int32_t)b.p;
      out.bits_sets.push_back(b);
      continue;
    }
    if (stage_is_multi(*q, o.bits_ok)) {
      out.shape.pk_cnt[i] = 0;
      MultiSet m;
      m.out = (int32_t)i;
      m.first_part = (uint32_t)out.multi_parts.size();
      uint32_t ids[LSG_MAX_SET_COMMITTEES], lens[LSG_MAX_SET_COMMITTEES];
      const uint32_t k = multi_set_ok(*q) ? multi_k(*q) : 0;
      bool ok = multi_set_ok(*q) && (k > 0 || q->n_pks == 0);
      uint64_t total = 0;
      if (ok && k) memcpy(ids, q->pks + 4, 4 * (size_t)k);
      for (uint32_t e = 0; e < k && ok; e++) {
        ok = cm.has(ids[e]);
        if (ok) total += (lens[e] = cm.len[ids[e]]);
      }
      if (!ok || total != q->n_pks)
        out.shape.bits_kerr[i] = LSG_ERR_BAD_COMMITTEE;
      else
        m = multi_stage_set(ids, lens, k, q->pks + 4 + 4 * (size_t)k, q->n_pks, (int32_t)i, cbits, &bw, out.multi_parts);
      out.shape.bits_p[i] = (int32_t)m.p;
      out.multi_sets.push_back(m);
      continue;
    }
    out.shape.pk_cnt[i] = q->n_pks;
    if (q->n_pks != 1) single = false;
    if (all_index) {  // the set's indices are contiguous in the caller's buffer
      std::fill(pklen + po, pklen + po + q->n_pks, (uint32_t)LSG_PK_INDEX);
      if (q->pks)
        memcpy(A + L.pk + 4 * po, q->pks, 4 * (size_t)q->n_pks);
      else
        memset(A + L.pk + 4 * po, 0, 4 * (size_t)q->n_pks);
      po += q->n_pks;
      continue;
    }
    for (uint32_t k = 0; k < q->n_pks; k++) {  // a slot of an unknown length or without bytes: zeroed
      pklen[po] = q->pk_len;
      uint8_t* pd = A + L.pk + 96 * po;
      if ((q->pk_len == 48 || q->pk_len == 96 || q->pk_len == LSG_PK_INDEX) && q->pks)
        memcpy(pd, q->pks + (size_t)q->pk_len * k, q->pk_len);
      else
        memset(pd, 0, 4);
      po++;
    }
  }
  out.single_keys = single && n > 0;
  out.n_msgs = nm;
  out.msg_used = mo;
  out.bit_words = bw;
  out.msg_objs = mc ? miss_obj : z.any_obj;
  out.msg_vars = mc ? miss_var : z.any_var;
  if (mc) {  // the source words of the nm distinct messages stay; the store's pairs follow them
    plan.resize(out.mc_src_off + nm);
    out.mc_st_off = plan.size();
    plan.insert(plan.end(), out.mc_store.begin(), out.mc_store.end());
  }
  out.msg_dedup = nm < n;
  if (out.msg_dedup) out.msg_id.assign(mid, mid + n);
  const int rc = draw_randomizers(rnd, n, o.scale, o.rnd_in, o.seed, o.noscale, entropy);
  if (rc) return rc;
  if (n) memcpy(out.rnd.data(), rnd, 8 * n);
  return LSG_OK;
}

}  // namespace lsgp
