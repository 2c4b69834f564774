// msgcachecheck.cpp -- CPU driver of the message-cache policy in
// lodestar_amd/csrc/lsg_msg_cache.hpp (tests/test_msg_cache_host.py).  No device: the class
// deals in keys, bytes and row numbers only.  The caller passes every message's 64-bit key in,
// so a script can give different messages one key.
//
//   msgcachecheck SCRIPT OUT    SCRIPT: whitespace-separated integers, OUT: one line per op
//
// SCRIPT = capacity n_ops, then per op its kind:
//   0 lookup   key len_word n_bytes bytes...   -> "L result row"   (0 hit, 1 pending, 2 miss; row -1 unless hit)
//   1 allot    key len_word n_bytes bytes...   -> "A ok row"       (row -1 unless ok)
//   2 unpin    stale n rows...                 -> "U"              (stale: epochs before the current one)
//   3 publish  stale n rows...                 -> "P"
//   4 drop     stale n rows...                 -> "D"
//   5 clear                                    -> "C"
//   6 stats                                    -> "S lookups hits pending inserts evictions bypassed full entries capacity"
//   7 bypass                                   -> "B"
//   8 resize   capacity                        -> "R"
//   9 threads  n_msgs iters                    -> "T rows_left lookups hits pending inserts full entries" after two
//              threads ran `iters` rounds each of lookup (+ allot on a miss), then publish (every 7th round: drop)
//              and unpin, over n_msgs shared messages; rows_left: rows still pinned or pending afterwards
// Any broken invariant prints a message and exits nonzero.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <fstream>
#include <string>
#include <thread>

#include "../../lodestar_amd/csrc/lsg_msg_cache.hpp"

using namespace lsgp;

namespace {

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "msgcachecheck: %s\n", m.c_str());
  exit(2);
}
#define REQUIRE(c, m) \
  do {                \
    if (!(c)) die(m); \
  } while (0)

struct Input {
  std::vector<long long> v;
  size_t at = 0;
  long long next() {
    REQUIRE(at < v.size(), "script ends early");
    return v[at++];
  }
};

struct Msg {
  uint64_t key;
  uint32_t len_word, n_bytes;
  std::vector<uint8_t> bytes;
};
Msg read_msg(Input& in) {
  Msg m;
  m.key = (uint64_t)in.next();
  m.len_word = (uint32_t)in.next();
  m.n_bytes = (uint32_t)in.next();
  REQUIRE(m.n_bytes <= 4096, "message too long for the driver");
  m.bytes.resize(m.n_bytes + 1);  // (exact size + 1: an overread of the caller's bytes is ASan's to find)
  for (uint32_t k = 0; k < m.n_bytes; k++) m.bytes[k] = (uint8_t)in.next();
  m.bytes.resize(m.n_bytes);
  m.bytes.shrink_to_fit();
  return m;
}
std::vector<uint32_t> read_rows(Input& in) {
  std::vector<uint32_t> r((size_t)in.next());
  for (uint32_t& x : r) x = (uint32_t)in.next();
  return r;
}

// two threads over shared messages: whatever one thread hits must be visible (published by a
// completed round), and a round's own allotted rows are never returned to the other thread
// before it publishes them
std::atomic<int> g_bad{0};
void worker(MsgCache* mc, int id, int n_msgs, int iters, std::vector<std::atomic<int>>* writing) {
  uint64_t rng = 0x9e3779b97f4a7c15ull * (uint64_t)(id + 1);
  for (int it = 0; it < iters; it++) {
    std::vector<uint32_t> pins, pend;
    const uint64_t epoch = mc->epoch();
    for (int k = 0; k < 3; k++) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint32_t m = (uint32_t)((rng >> 33) % (uint64_t)n_msgs);
      uint8_t bytes[8];
      memcpy(bytes, &m, 4);
      memcpy(bytes + 4, &m, 4);
      uint32_t row = 0;
      const uint64_t key = m & 3;  // (four buckets' worth of keys: chains and equal keys)
      const MsgCache::Result r = mc->lookup(key, bytes, 8, 8, &row);
      if (r == MsgCache::HIT) {
        if ((*writing)[row].load()) g_bad++;  // a row being written was returned
        pins.push_back(row);
      } else if (r == MsgCache::MISS && mc->allot(key, bytes, 8, 8, &row)) {
        if ((*writing)[row].fetch_add(1) != 0) g_bad++;  // two writers of one row
        pend.push_back(row);
      }
    }
    std::this_thread::yield();
    for (uint32_t r : pend) (*writing)[r].fetch_sub(1);
    mc->unpin(epoch, pins.data(), pins.size());
    if (it % 7 == 6)
      mc->drop(epoch, pend.data(), pend.size());
    else
      mc->publish(epoch, pend.data(), pend.size());
  }
}

}  // namespace

int main(int argc, char** argv) {
  REQUIRE(argc == 3, "usage: msgcachecheck SCRIPT OUT");
  Input in;
  {
    std::ifstream f(argv[1]);
    REQUIRE(f.good(), "cannot read the script");
    long long x;
    while (f >> x) in.v.push_back(x);
  }
  FILE* out = fopen(argv[2], "w");
  REQUIRE(out != nullptr, "cannot write the output");
  MsgCache mc;
  mc.resize((size_t)in.next());
  const long long n_ops = in.next();
  for (long long op = 0; op < n_ops; op++) {
    const int kind = (int)in.next();
    if (kind == 0 || kind == 1) {
      const Msg m = read_msg(in);
      uint32_t row = 0xffffffffu;
      if (kind == 0) {
        const MsgCache::Result r = mc.lookup(m.key, m.bytes.data(), m.len_word, m.n_bytes, &row);
        fprintf(out, "L %d %lld\n", (int)r, r == MsgCache::HIT ? (long long)row : -1ll);
      } else {
        const bool ok = mc.allot(m.key, m.bytes.data(), m.len_word, m.n_bytes, &row);
        fprintf(out, "A %d %lld\n", ok ? 1 : 0, ok ? (long long)row : -1ll);
      }
    } else if (kind >= 2 && kind <= 4) {
      const uint64_t epoch = mc.epoch() - (uint64_t)in.next();
      const std::vector<uint32_t> rows = read_rows(in);
      if (kind == 2) mc.unpin(epoch, rows.data(), rows.size());
      if (kind == 3) mc.publish(epoch, rows.data(), rows.size());
      if (kind == 4) mc.drop(epoch, rows.data(), rows.size());
      fprintf(out, "%c\n", "UPD"[kind - 2]);
    } else if (kind == 5) {
      mc.clear();
      fprintf(out, "C\n");
    } else if (kind == 6) {
      const MsgCacheStats s = mc.stats();
      fprintf(out, "S %llu %llu %llu %llu %llu %llu %llu %u %u\n", (unsigned long long)s.lookups,
              (unsigned long long)s.hits, (unsigned long long)s.pending, (unsigned long long)s.inserts,
              (unsigned long long)s.evictions, (unsigned long long)s.bypassed, (unsigned long long)s.full, s.entries,
              s.capacity);
    } else if (kind == 7) {
      mc.note_bypass();
      fprintf(out, "B\n");
    } else if (kind == 8) {
      mc.resize((size_t)in.next());
      fprintf(out, "R\n");
    } else if (kind == 9) {
      const int n_msgs = (int)in.next(), iters = (int)in.next();
      std::vector<std::atomic<int>> writing(mc.capacity());
      for (auto& w : writing) w.store(0);
      std::thread a(worker, &mc, 0, n_msgs, iters, &writing), b(worker, &mc, 1, n_msgs, iters, &writing);
      a.join();
      b.join();
      REQUIRE(g_bad.load() == 0, "a pending row was returned by a lookup, or allotted twice");
      const MsgCacheStats st = mc.stats();
      // nothing stays pinned or pending: capacity fresh messages all find a row
      int left = 0;
      std::vector<uint32_t> rows;
      for (uint32_t k = 0; k < mc.capacity(); k++) {
        uint8_t bytes[8];
        const uint64_t v = 0xabcdef0000000000ull + k;
        memcpy(bytes, &v, 8);
        uint32_t row = 0;
        if (mc.allot(v, bytes, 8, 8, &row))
          rows.push_back(row);
        else
          left++;
      }
      mc.drop(mc.epoch(), rows.data(), rows.size());
      fprintf(out, "T %d %llu %llu %llu %llu %llu %u\n", left, (unsigned long long)st.lookups, (unsigned long long)st.hits,
              (unsigned long long)st.pending, (unsigned long long)st.inserts, (unsigned long long)st.full, st.entries);
    } else {
      die("unknown op " + std::to_string(kind));
    }
  }
  fclose(out);
  return 0;
}
