// lsg_msg_cache.hpp -- the host policy of the message cache (lsg_msg_cache_set):
// which staged message owns which row of a device's arena of hash_to_G2 points, when a row may
// be read, and which row a new message takes.  Bytes and small integers in, row numbers out: no
// device, no Slot, no pointers into callers' buffers (key bytes are copied into a flat store).
// lsg_host.hip keeps one per device and supplies the device side (k_h2c_cache_merge,
// k_h2c_cache_store); tests/native/msgcachecheck.cpp drives it on the CPU.
//
// A row is FREE, PENDING (allotted to a launch that is writing it: never returned by a lookup,
// never evicted) or VISIBLE (published once the host has observed that launch's completion).
// A launch pins the visible rows it reads; a pinned row is never evicted.  Replacement is
// CLOCK: a hit sets the row's referenced bit, the hand passes a referenced row once and clears
// the bit.  clear() and resize() start a new epoch: what a launch staged in an earlier epoch
// (its pins, its pending rows) is void: unpin(), publish() and drop() of such a launch change nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

namespace lsgp {

constexpr uint32_t MSG_CACHE_MAX_BYTES = 192;  // longer staged messages (and empty ones) bypass the cache

struct MsgCacheStats {
  uint64_t lookups = 0, hits = 0, pending = 0, inserts = 0, evictions = 0, bypassed = 0, full = 0;
  uint32_t entries = 0, capacity = 0;
};

class MsgCache {
 public:
  enum Result { HIT = 0, PENDING = 1, MISS = 2 };

  // `capacity` rows, every one free; counters zeroed (0: off, the stores released)
  void resize(size_t capacity) {
    std::lock_guard<std::mutex> lk(mu_);
    cap_ = (uint32_t)capacity;
    rows_.assign(capacity, Row());
    bytes_.assign(capacity * MSG_CACHE_MAX_BYTES, 0);
    size_t nb = 1;
    while (capacity && nb < 2 * capacity) nb <<= 1;
    head_.assign(capacity ? nb : 0, NONE);
    if (!capacity) {
      rows_.shrink_to_fit();
      bytes_.shrink_to_fit();
      head_.shrink_to_fit();
    }
    hand_ = busy_ = 0;
    epoch_++;
    st_ = MsgCacheStats();
    st_.capacity = cap_;
  }

  // every entry dropped (counters stay)
  void clear() {
    std::lock_guard<std::mutex> lk(mu_);
    for (Row& r : rows_) r = Row();
    std::fill(head_.begin(), head_.end(), NONE);
    hand_ = busy_ = 0;
    epoch_++;
    st_.entries = 0;
  }

  uint32_t capacity() const { return cap_; }
  uint64_t epoch() {
    std::lock_guard<std::mutex> lk(mu_);
    return epoch_;
  }
  static bool cacheable(uint32_t n_bytes) { return n_bytes > 0 && n_bytes <= MSG_CACHE_MAX_BYTES; }
  void note_bypass() {
    std::lock_guard<std::mutex> lk(mu_);
    st_.bypassed++;
  }

  // The message (key: the caller's 64-bit mix, which selects the bucket only; len_word: its
  // length as staged, marker included; n_bytes payload bytes at `m`).  HIT: *row is pinned for
  // the caller's launch and marked referenced.  PENDING: another launch is writing it.  MISS:
  // unknown -- the caller hashes it and may allot() a row.
  Result lookup(uint64_t key, const uint8_t* m, uint32_t len_word, uint32_t n_bytes, uint32_t* row) {
    std::lock_guard<std::mutex> lk(mu_);
    st_.lookups++;
    const uint32_t r = find(key, m, len_word, n_bytes);
    if (r == NONE) return MISS;
    if (rows_[r].state == ST_PENDING) {
      st_.pending++;
      return PENDING;
    }
    if (rows_[r].pins++ == 0) busy_++;
    rows_[r].ref = 1;
    st_.hits++;
    *row = r;
    return HIT;
  }

  // A row for a message whose lookup() missed (the same arguments): true and *row, PENDING
  // until publish().  false: every row is pinned or pending (`full`), or another
  // thread allotted the message since the lookup (`pending`) -- hash it and store nothing.
  bool allot(uint64_t key, const uint8_t* m, uint32_t len_word, uint32_t n_bytes, uint32_t* row) {
    std::lock_guard<std::mutex> lk(mu_);
    if (find(key, m, len_word, n_bytes) != NONE) {
      st_.pending++;
      return false;
    }
    // every row pinned or pending: the sweep below would pass over them all and change nothing
    // (a package of thousands of new messages asks thousands of times)
    if (busy_ == cap_) {
      st_.full++;
      return false;
    }
    // a row that is neither is free, or visible and at the latest in the second round unreferenced
    for (uint32_t step = 0; step < 2 * cap_; step++) {
      const uint32_t r = hand_;
      hand_ = hand_ + 1 == cap_ ? 0 : hand_ + 1;
      Row& R = rows_[r];
      if (R.state == ST_PENDING || R.pins) continue;
      if (R.state == ST_VISIBLE) {
        if (R.ref) {  // its second chance
          R.ref = 0;
          continue;
        }
        unlink(r);
        st_.evictions++;
        st_.entries--;
      }
      R = Row();
      R.state = ST_PENDING;
      busy_++;
      R.key = key;
      R.len_word = len_word;
      R.n_bytes = n_bytes;
      memcpy(bytes_.data() + (size_t)r * MSG_CACHE_MAX_BYTES, m, n_bytes);
      const size_t b = bucket(key);
      R.next = head_[b];
      head_[b] = r;
      st_.inserts++;
      *row = r;
      return true;
    }
    st_.full++;
    return false;
  }

  // A launch staged in `epoch` is over (the three calls below).  unpin: the rows its lookups hit.
  void unpin(uint64_t epoch, const uint32_t* rows, size_t n) {
    std::lock_guard<std::mutex> lk(mu_);
    if (epoch != epoch_) return;
    for (size_t i = 0; i < n; i++)
      if (rows[i] < cap_ && rows_[rows[i]].pins && --rows_[rows[i]].pins == 0) busy_--;
  }
  // publish: the host observed the launch's completion -- the rows it allotted become visible
  void publish(uint64_t epoch, const uint32_t* rows, size_t n) {
    std::lock_guard<std::mutex> lk(mu_);
    if (epoch != epoch_) return;
    for (size_t i = 0; i < n; i++) {
      if (rows[i] >= cap_ || rows_[rows[i]].state != ST_PENDING) continue;
      rows_[rows[i]].state = ST_VISIBLE;
      busy_--;
      st_.entries++;
    }
  }
  // drop: the submit failed -- the rows it allotted are free again
  void drop(uint64_t epoch, const uint32_t* rows, size_t n) {
    std::lock_guard<std::mutex> lk(mu_);
    if (epoch != epoch_) return;
    for (size_t i = 0; i < n; i++) {
      if (rows[i] >= cap_ || rows_[rows[i]].state != ST_PENDING) continue;
      unlink(rows[i]);
      rows_[rows[i]] = Row();
      busy_--;
    }
  }

  MsgCacheStats stats() {
    std::lock_guard<std::mutex> lk(mu_);
    return st_;
  }

 private:
  enum : uint8_t { ST_FREE = 0, ST_PENDING = 1, ST_VISIBLE = 2 };
  static constexpr uint32_t NONE = 0xffffffffu;
  struct Row {
    uint64_t key = 0;
    uint32_t len_word = 0, n_bytes = 0;
    uint32_t pins = 0;
    uint32_t next = NONE;  // the bucket's chain
    uint8_t state = ST_FREE, ref = 0;
  };
  size_t bucket(uint64_t key) const { return (size_t)key & (head_.size() - 1); }
  uint32_t find(uint64_t key, const uint8_t* m, uint32_t len_word, uint32_t n_bytes) const {
    if (!cap_) return NONE;
    for (uint32_t r = head_[bucket(key)]; r != NONE; r = rows_[r].next) {
      const Row& R = rows_[r];
      if (R.key == key && R.len_word == len_word && R.n_bytes == n_bytes &&
          memcmp(bytes_.data() + (size_t)r * MSG_CACHE_MAX_BYTES, m, n_bytes) == 0)
        return r;
    }
    return NONE;
  }
  void unlink(uint32_t r) {
    uint32_t* p = &head_[bucket(rows_[r].key)];
    while (*p != NONE && *p != r) p = &rows_[*p].next;
    if (*p == r) *p = rows_[r].next;
  }

  std::mutex mu_;
  uint32_t cap_ = 0, hand_ = 0;
  uint32_t busy_ = 0;  // rows pinned or pending: none of them can be handed out
  uint64_t epoch_ = 0;
  std::vector<Row> rows_;
  std::vector<uint8_t> bytes_;  // row r's key bytes at r * MSG_CACHE_MAX_BYTES
  std::vector<uint32_t> head_;  // bucket -> first row of its chain
  MsgCacheStats st_;
};

}  // namespace lsgp
