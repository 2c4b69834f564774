// stagecheck.cpp -- CPU driver of package staging in lodestar_amd/csrc/lsg_stage.hpp and of the
// two plan lists of lsg_plan.hpp that follow it in a package (tests/test_stage_host.py).  No
// device: the staging arena is a malloc of exactly StageLayout::bytes, the bit arena one of
// exactly the measured words, every caller buffer (signature, message, key blob) one of exactly
// its stated length, so a write or read past a promise is AddressSanitizer's to find.  Both
// arenas are filled with 0xa5 first: what staging leaves untouched shows in the output.  One
// Staged and one MsgTable serve every case of a script, as a pipeline slot's serve its packages.
//
//   stagecheck SCRIPT OUT    SCRIPT: whitespace-separated unsigned integers
//
// SCRIPT = n_cases, then per case its kind:
//   1 layout   n npk stride msg_bytes           -> "layout ..." (the nine offsets, the size)
//   0 stage:
//     n_committees, per id: ok len
//     cache: given capacity n_ops, per op: kind (0 lookup, 1 allot, 2 unpin, 3 publish) and
//            key len_word n_bytes bytes... (0, 1) or n rows... (2, 3)
//     scale dedup dedup_on bits_ok seed keymode plan_prefix
//     entropy: n_calls, per call: ok n_words words...
//     jobs: n_jobs (0: the sets as listed), per job: flags n_sets
//     msg_lists: want first len              (plan_msg_lists over sets [first, first + len))
//     n_sets, per set: sig_len present n_bytes bytes... | msg_len present n_bytes bytes...
//                      | n_pks pk_len present n_bytes bytes... | noscale(0/1/2: no list) rnd_in key
//   keymode 1: the per-set `key` replaces msg_key (different messages on one key); rnd_in is
//   used when the first set's is nonzero.
// OUT: per case lines "name values..." ending in "end" (see main).
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <map>
#include <string>

#include "../../lodestar_amd/csrc/lsg_stage.hpp"

using namespace lsgp;

namespace {

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "stagecheck: %s\n", m.c_str());
  exit(2);
}
#define REQUIRE(c, m) \
  do {                \
    if (!(c)) die(m); \
  } while (0)

struct Input {
  std::vector<uint64_t> v;
  size_t at = 0;
  uint64_t next() {
    REQUIRE(at < v.size(), "script ends early");
    return v[at++];
  }
};

// a caller buffer of exactly n bytes (null when absent)
struct Buf {
  uint8_t* p = nullptr;
  Buf() {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  void read(Input& in) {
    const bool present = in.next() != 0;
    const size_t n = (size_t)in.next();
    REQUIRE(n <= (1u << 20), "buffer too long for the driver");
    if (!present) {
      REQUIRE(n == 0, "bytes of an absent buffer");
      return;
    }
    p = (uint8_t*)malloc(n);  // (n == 0: a present buffer of no bytes, none of them readable)
    REQUIRE(p != nullptr, "malloc");
    for (size_t k = 0; k < n; k++) p[k] = (uint8_t)in.next();
  }
  ~Buf() { free(p); }
};

template <class T>
void line(FILE* out, const char* name, const T* v, size_t n) {
  fprintf(out, "%s", name);
  for (size_t k = 0; k < n; k++) fprintf(out, " %lld", (long long)v[k]);
  fprintf(out, "\n");
}
void line_u64(FILE* out, const char* name, const uint64_t* v, size_t n) {
  fprintf(out, "%s", name);
  for (size_t k = 0; k < n; k++) fprintf(out, " %llu", (unsigned long long)v[k]);
  fprintf(out, "\n");
}
void line_hex(FILE* out, const char* name, const uint8_t* v, size_t n) {
  fprintf(out, "%s ", name);
  for (size_t k = 0; k < n; k++) fprintf(out, "%02x", v[k]);
  fprintf(out, "\n");
}
void print_layout(FILE* out, const StageLayout& L) {
  const long long v[] = {(long long)L.sig,   (long long)L.siglen, (long long)L.msgoff, (long long)L.msglen, (long long)L.mid,
                         (long long)L.pklen, (long long)L.rnd,    (long long)L.pk,     (long long)L.msg,    (long long)L.bytes};
  line(out, "layout", v, 10);
}

struct EntropyScript {
  struct Call {
    bool ok;
    std::vector<uint64_t> words;
  };
  std::vector<Call> calls;
  size_t at = 0;
  bool operator()(void* buf, size_t len) {
    REQUIRE(at < calls.size(), "more entropy calls than the script has");
    const Call& c = calls[at++];
    if (!c.ok) return false;
    REQUIRE(len == 8 * c.words.size(), "an entropy call of another length than the script's");
    memcpy(buf, c.words.data(), len);
    return true;
  }
};

void stage_case(Input& in, FILE* out, Staged& st, MsgTable& mt) {
  std::vector<uint32_t> cm_len;
  std::vector<uint8_t> cm_ok;
  for (size_t k = (size_t)in.next(); k; k--) {
    cm_ok.push_back((uint8_t)in.next());
    cm_len.push_back((uint32_t)in.next());
  }
  // (exact sizes: a read past the registry is ASan's to find)
  cm_len.shrink_to_fit();
  cm_ok.shrink_to_fit();
  const bool mc_given = in.next() != 0;
  MsgCache mc;
  mc.resize((size_t)in.next());
  for (size_t ops = (size_t)in.next(); ops; ops--) {
    const int kind = (int)in.next();
    if (kind <= 1) {
      const uint64_t key = in.next();
      const uint32_t len_word = (uint32_t)in.next();
      std::vector<uint8_t> b((size_t)in.next());
      for (uint8_t& x : b) x = (uint8_t)in.next();
      uint32_t row = 0;
      if (kind == 0)
        (void)mc.lookup(key, b.data(), len_word, (uint32_t)b.size(), &row);
      else
        (void)mc.allot(key, b.data(), len_word, (uint32_t)b.size(), &row);
    } else {
      std::vector<uint32_t> rows((size_t)in.next());
      for (uint32_t& r : rows) r = (uint32_t)in.next();
      if (kind == 2) mc.unpin(mc.epoch(), rows.data(), rows.size());
      if (kind == 3) mc.publish(mc.epoch(), rows.data(), rows.size());
    }
  }
  StageOpts o;
  o.scale = in.next() != 0;
  o.dedup = in.next() != 0;
  o.dedup_on = in.next() != 0;
  o.bits_ok = in.next() != 0;
  o.seed = in.next();
  const bool keymode = in.next() != 0;
  std::vector<int32_t> plan((size_t)in.next(), 7);
  EntropyScript ent;
  for (size_t k = (size_t)in.next(); k; k--) {
    EntropyScript::Call c;
    c.ok = in.next() != 0;
    c.words.resize((size_t)in.next());
    for (uint64_t& w : c.words) w = in.next();
    ent.calls.push_back(c);
  }
  std::vector<lsg_job> jobs((size_t)in.next());
  for (lsg_job& J : jobs) {
    J.flags = (uint32_t)in.next();
    J.n_sets = (uint32_t)in.next();
    J.sets = nullptr;
  }
  const bool want_lists = in.next() != 0;
  Grp lists_g;
  lists_g.first = (size_t)in.next();
  lists_g.len = (size_t)in.next();
  const size_t n = (size_t)in.next();
  std::vector<lsg_set> sets(n);
  std::vector<Buf> sig(n), msg(n), pks(n);
  std::vector<uint8_t> noscale;
  std::vector<uint64_t> rnd_in(n);
  std::map<const lsg_set*, uint64_t> keys;
  bool has_noscale = false;
  for (size_t i = 0; i < n; i++) {
    lsg_set& t = sets[i];
    t.sig_len = (uint32_t)in.next();
    sig[i].read(in);
    t.sig = sig[i].p;
    t.msg_len = (uint32_t)in.next();
    msg[i].read(in);
    t.msg = msg[i].p;
    t.n_pks = (uint32_t)in.next();
    t.pk_len = (uint32_t)in.next();
    pks[i].read(in);
    t.pks = pks[i].p;
    const uint64_t ns = in.next();
    has_noscale = has_noscale || ns != 2;
    noscale.push_back(ns == 1);
    rnd_in[i] = in.next();
    keys[&t] = in.next();
  }
  // staging order: the sets as listed, or the jobs' (batchable jobs first, as pkg_part1 does it)
  std::vector<const lsg_set*> flat(n);
  st.shape.jobs.clear();
  if (jobs.empty()) {
    for (size_t i = 0; i < n; i++) flat[i] = &sets[i];
  } else {
    size_t at = 0;
    std::vector<size_t> ids;
    for (size_t j = 0; j < jobs.size(); j++) {
      jobs[j].sets = sets.data() + at;
      at += jobs[j].n_sets;
      ids.push_back(j);
    }
    REQUIRE(at == n, "the jobs' sets are not the sets listed");
    REQUIRE(shape_jobs(st.shape, jobs.data(), ids, nullptr) == n, "shape_jobs counts other sets");
    for (size_t k = 0; k < jobs.size(); k++)
      for (uint32_t q = 0; q < jobs[k].n_sets; q++) flat[st.shape.jobs[k].first + q] = &jobs[k].sets[q];
    // (the per-set script columns follow the sets into staging order)
    std::vector<uint8_t> ns2(n);
    std::vector<uint64_t> r2(n);
    for (size_t i = 0; i < n; i++) {
      ns2[i] = noscale[(size_t)(flat[i] - sets.data())];
      r2[i] = rnd_in[(size_t)(flat[i] - sets.data())];
    }
    noscale = ns2;
    rnd_in = r2;
  }
  if (has_noscale) o.noscale = &noscale;
  if (n && rnd_in[0]) o.rnd_in = rnd_in.data();

  const StageSizes z = stage_measure(flat.data(), n, o.bits_ok);
  {
    const long long v[] = {(long long)z.npk,       (long long)z.msg_total, (long long)z.n_bits_sets, (long long)z.n_multi,
                           (long long)z.bit_words, z.all_index ? 1 : 0,    z.any_obj ? 1 : 0};
    line(out, "sizes", v, 7);
  }
  const StageLayout L = stage_layout(n, z.npk, z.pk_stride(), z.msg_total);
  print_layout(out, L);
  uint8_t* A = (uint8_t*)malloc(L.bytes);
  uint32_t* cbits = (uint32_t*)malloc(z.bit_words ? 4 * z.bit_words : 1);
  REQUIRE(A && cbits, "malloc");
  if (!z.bit_words) {  // no word promised: none may be touched
    free(cbits);
    cbits = nullptr;
  }
  memset(A, 0xa5, L.bytes);
  if (cbits) memset(cbits, 0xa5, 4 * z.bit_words);
  const Committees cm{cm_len.data(), cm_ok.data(), cm_ok.size()};
  int rc;
  if (keymode)
    rc = stage_fill(A, L, cbits, flat.data(), n, z, o, mc_given ? &mc : nullptr, cm, mt, plan, st,
                    [&](const lsg_set& t) { return keys.at(&t); }, ent);
  else
    rc = stage_fill(A, L, cbits, flat.data(), n, z, o, mc_given ? &mc : nullptr, cm, mt, plan, st, MsgKey(), ent);
  fprintf(out, "rc %d\n", rc);
  fprintf(out, "entropy_calls %zu\n", ent.at);
  {
    const long long v[] = {(long long)st.n_sets,  (long long)st.n_pks,      (long long)st.pk_stride,  (long long)st.n_msgs,
                           st.msg_dedup ? 1 : 0,  st.msg_objs ? 1 : 0,      st.single_keys ? 1 : 0,   st.pk_all_bits ? 1 : 0,
                           st.mc_on ? 1 : 0,      (long long)st.n_miss,     (long long)st.mc_hits,    (long long)st.mc_src_off,
                           (long long)st.mc_st_off, (long long)st.msg_used, (long long)st.bit_words,  (long long)st.mc_epoch};
    line(out, "res", v, 16);
  }
  REQUIRE(st.bit_words <= z.bit_words, "more bit words used than measured");
  REQUIRE(st.msg_used <= z.msg_total, "more message bytes used than measured");
  if (rc == LSG_OK) line_u64(out, "rnd", st.rnd.data(), st.rnd.size());
  if (st.msg_dedup) line(out, "msg_id", st.msg_id.data(), st.msg_id.size());
  line(out, "pins", st.mc_pins.data(), st.mc_pins.size());
  line(out, "pend", st.mc_pend.data(), st.mc_pend.size());
  line(out, "store", st.mc_store.data(), st.mc_store.size());
  line(out, "pk_cnt", st.shape.pk_cnt.data(), st.shape.pk_cnt.size());
  line(out, "pk_first", st.shape.pk_first.data(), st.shape.pk_first.size());
  line(out, "bits_p", st.shape.bits_p.data(), st.shape.bits_p.size());
  line(out, "bits_kerr", st.shape.bits_kerr.data(), st.shape.bits_kerr.size());
  fprintf(out, "bits_sets");
  for (const BitsSet& b : st.bits_sets) fprintf(out, " %u %u %u %u %d", b.committee, b.word_off, b.n_bits, b.p, b.out);
  fprintf(out, "\nmulti_sets");
  for (const MultiSet& m : st.multi_sets) fprintf(out, " %u %u %u %u %d", m.first_part, m.n_parts, m.p, m.items, m.out);
  fprintf(out, "\nmulti_parts");
  for (const MultiPart& q : st.multi_parts) fprintf(out, " %u %u %u %u", q.committee, q.word_off, q.n_bits, q.p);
  fprintf(out, "\n");
  // the arena, read through the layout
  line(out, "a_siglen", (const uint32_t*)(A + L.siglen), L.nn);
  line(out, "a_msgoff", (const uint32_t*)(A + L.msgoff), L.nn);
  line(out, "a_msglen", (const uint32_t*)(A + L.msglen), L.nn);
  line(out, "a_mid", (const uint32_t*)(A + L.mid), L.nn);
  line(out, "a_pklen", (const uint32_t*)(A + L.pklen), L.np);
  line_u64(out, "a_rnd", (const uint64_t*)(A + L.rnd), L.nn);
  line_hex(out, "a_sig", A + L.sig, 192 * L.nn);
  line_hex(out, "a_pk", A + L.pk, L.stride * L.np);
  line_hex(out, "a_msg", A + L.msg, L.mb);
  line(out, "cbits", cbits, z.bit_words);
  {
    const MsgCacheStats s = mc.stats();
    const long long v[] = {(long long)s.lookups,   (long long)s.hits,     (long long)s.pending, (long long)s.inserts,
                           (long long)s.evictions, (long long)s.bypassed, (long long)s.full,    (long long)s.entries};
    line(out, "mcstats", v, 8);
  }
  // what pkg_part1 appends next: the KeyValidate list, the package group's per-message lists
  if (!jobs.empty() && rc == LSG_OK) {
    size_t kv_off = 0;
    const size_t n_kv = plan_validate_keys(st.shape, flat.data(), n, plan, &kv_off);
    fprintf(out, "kv %zu %zu\n", n_kv, n_kv ? kv_off : (size_t)0);
    line(out, "kv_set", st.shape.kv_set.data(), st.shape.kv_set.size());
  }
  if (want_lists && rc == LSG_OK) {
    REQUIRE(st.msg_dedup && lists_g.first + lists_g.len <= n, "per-message lists of a package without repeats");
    const SegPlan P = plan_msg_lists(plan, st.msg_id.data(), st.n_msgs, lists_g, SEG_FOLD_WIDE);
    fprintf(out, "msum %d %d %zu %zu %zu", P.op, P.has_idx ? 1 : 0, P.idx_off, P.tmp_items, P.passes.size());
    for (const SegPass& p : P.passes) fprintf(out, " %d %d %zu %d %d", p.ips_log2, p.n_chunks, p.chunk_off, p.src, p.tmp_out);
    fprintf(out, "\n");
  }
  line(out, "plan", plan.data(), plan.size());
  fprintf(out, "end\n");
  free(A);
  free(cbits);
}

}  // namespace

int main(int argc, char** argv) {
  REQUIRE(argc == 3, "usage: stagecheck SCRIPT OUT");
  Input in;
  {
    std::ifstream f(argv[1]);
    REQUIRE(f.good(), "cannot read the script");
    unsigned long long x;
    while (f >> x) in.v.push_back(x);
  }
  FILE* out = fopen(argv[2], "w");
  REQUIRE(out != nullptr, "cannot write the output");
  Staged st;
  MsgTable mt;
  for (uint64_t cases = in.next(); cases; cases--) {
    const int kind = (int)in.next();
    if (kind == 1) {
      const size_t n = (size_t)in.next(), npk = (size_t)in.next(), stride = (size_t)in.next(), mb = (size_t)in.next();
      print_layout(out, stage_layout(n, npk, stride, mb));
      fprintf(out, "end\n");
    } else if (kind == 0) {
      stage_case(in, out, st, mt);
    } else {
      die("unknown case kind " + std::to_string(kind));
    }
  }
  REQUIRE(in.at == in.v.size(), "script has words left over");
  fclose(out);
  return 0;
}
