// sszcheck.cpp -- CPU driver of the SSZ signing roots (lodestar_amd/csrc/lsg_ssz.hpp: the text
// k_msg_roots and the signing-root kernels run on the device) and of the host policy of
// LSG_MSG_OBJECT sets in lodestar_amd/csrc/lsg_plan.hpp (payload length -> kind, the argument
// check).  Built with AddressSanitizer and UBSan by tests/test_ssz_roots_host.py, which compares
// every root with oracle/interop.py.
//
//   sszcheck roots IN OUT   IN: one case per line, "<object hex> <domain hex>"; OUT: per case the
//                           root in hex, once stored to a buffer of its own and once over the
//                           start of object || domain, as k_msg_roots stores it ("-" for a
//                           length that names no kind)
//   sszcheck classify       per line "<len> <kind unmarked> <kind marked>" for len 0..200
//   sszcheck args           the argument check on NULL messages and unknown lengths; prints "ok"
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/lsg_plan.hpp"
#include "../../lodestar_amd/csrc/lsg_ssz.hpp"

static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> b;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
    unsigned v = 0;
    sscanf(s + i, "%2x", &v);
    b.push_back((uint8_t)v);
  }
  return b;
}
static std::string hex(const uint8_t* p, size_t n) {
  std::string s;
  char t[3];
  for (size_t i = 0; i < n; i++) {
    snprintf(t, sizeof t, "%02x", p[i]);
    s += t;
  }
  return s;
}

static int run_roots(const char* in, const char* out) {
  FILE* fi = fopen(in, "r");
  FILE* fo = fopen(out, "w");
  if (!fi || !fo) return 2;
  static char a[1024], b[1024];
  while (fscanf(fi, "%1000s %1000s", a, b) == 2) {
    const std::vector<uint8_t> obj = unhex(a[0] == '-' ? "" : a), dom = unhex(b);
    if (dom.size() != 32) return 3;
    // exact-size heap buffers: a read or a store past either end is an ASan report
    std::vector<uint8_t> o(obj), d(dom), r(32, 0xaa);
    const bool ok = ssz_object_signing_root((uint32_t)o.size(), o.data(), d.data(), r.data());
    std::vector<uint8_t> payload(obj);
    payload.insert(payload.end(), dom.begin(), dom.end());
    const bool ok2 = ssz_object_signing_root((uint32_t)obj.size(), payload.data(), payload.data() + obj.size(), payload.data());
    if (ok != ok2) return 4;
    // the kind the stager admits for this payload is the one the dispatcher computes
    const uint32_t kind = lsgp::msg_object_kind(LSG_MSG_OBJECT | (uint32_t)(obj.size() + 32));
    if ((kind != 0) != ok || (ok && kind != obj.size())) return 5;
    if (!ok) {
      fprintf(fo, "- -\n");
      continue;
    }
    // only the first 32 bytes of the payload are written
    std::vector<uint8_t> before(obj);
    before.insert(before.end(), dom.begin(), dom.end());
    if (memcmp(payload.data() + 32, before.data() + 32, before.size() - 32)) return 6;
    fprintf(fo, "%s %s\n", hex(r.data(), 32).c_str(), hex(payload.data(), 32).c_str());
  }
  fclose(fi);
  fclose(fo);
  return 0;
}

static int run_classify() {
  for (uint32_t len = 0; len <= 200; len++)
    printf("%u %u %u %u %u\n", len, lsgp::msg_object_kind(len), lsgp::msg_object_kind(len | LSG_MSG_OBJECT),
           lsgp::msg_bytes(len | LSG_MSG_OBJECT), (unsigned)lsgp::msg_marked(len));
  return 0;
}

static int run_args() {
  const uint8_t buf[256] = {0};
  const uint32_t good[] = {40, 48, 64, 108, 120, 144, 160};
  lsg_set t;
  memset(&t, 0, sizeof t);
  // unmarked sets pass whatever they hold (NULL and odd lengths are data there)
  for (uint32_t len = 0; len <= 200; len++) {
    t.msg = len & 1 ? buf : nullptr;
    t.msg_len = len;
    if (!lsgp::msg_set_ok(t)) return 10;
  }
  for (uint32_t len = 0; len <= 200; len++) {
    bool in_table = false;
    for (uint32_t g : good) in_table = in_table || g == len;
    t.msg_len = len | LSG_MSG_OBJECT;
    t.msg = buf;
    if (lsgp::msg_set_ok(t) != in_table) return 11;
    t.msg = nullptr;  // a marked set without bytes is never accepted
    if (lsgp::msg_set_ok(t)) return 12;
  }
  // one bad set anywhere fails the package; jobs without sets are skipped
  std::vector<lsg_set> sets(5, t);
  for (lsg_set& q : sets) {
    q.msg = buf;
    q.msg_len = 32;
  }
  sets[1].msg_len = 160 | LSG_MSG_OBJECT;
  sets[3].msg_len = 40 | LSG_MSG_OBJECT;
  lsg_job jobs[3];
  jobs[0] = {sets.data(), 2, LSG_JOB_BATCHABLE};
  jobs[1] = {nullptr, 0, 0};
  jobs[2] = {sets.data() + 2, 3, 0};
  if (!lsgp::msg_sets_ok(sets.data(), sets.size()) || !lsgp::msg_jobs_ok(jobs, 3) || !lsgp::msg_jobs_ok(nullptr, 0)) return 13;
  sets[4].msg_len = 65 | LSG_MSG_OBJECT;
  if (lsgp::msg_sets_ok(sets.data(), sets.size()) || lsgp::msg_jobs_ok(jobs, 3) || !lsgp::msg_jobs_ok(jobs, 2)) return 14;
  sets[4].msg_len = 64 | LSG_MSG_OBJECT;
  sets[4].msg = nullptr;
  if (lsgp::msg_jobs_ok(jobs, 3)) return 15;
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "roots")) return run_roots(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "classify")) return run_classify();
  if (argc == 2 && !strcmp(argv[1], "args")) return run_args();
  fprintf(stderr, "usage: sszcheck roots IN OUT | classify | args\n");
  return 1;
}
