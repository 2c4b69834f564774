// sszvarcheck.cpp -- CPU driver of the variable-size LSG_MSG_OBJECT kinds
// (lodestar_amd/csrc/lsg_ssz.hpp: ssz_var_step, the text k_msg_roots_var runs with one 64-lane
// workgroup per object; altair.ContributionAndProof; the zero-subtree table) and of their host
// policy in lodestar_amd/csrc/lsg_plan.hpp (the length word's three fields, the structural
// check).  Built with AddressSanitizer and UBSan by tests/test_ssz_var_roots_host.py, which
// compares every root with tests/msgobjects_var.py.
//
// The driver steps 64 logical lanes phase by phase, as the kernel's barriers do: every lane of
// phase p runs before any lane of phase p + 1.  The dependent count it reports is the sum over
// the phases of the busiest lane's node hashes.
//
//   sszvarcheck roots IN OUT  IN: per line "<kind> <object hex> <domain hex>" (kind 0: tag 0, by
//                             length); OUT: per case "<root> <root over the payload> <dependent
//                             hashes> <bound>"
//   sszvarcheck zero          the ten zero-subtree hashes in hex
//   sszvarcheck classify      per tag 0..127: the fields of marked and unmarked words
//   sszvarcheck args          the structural check on exact-size buffers; prints "ok"
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

// one object through the phases; returns the dependent node hashes
static uint32_t var_root(uint32_t kind, const uint8_t* obj, uint32_t obj_len, const uint8_t* domain, uint8_t* out) {
  std::vector<uint32_t> nodes(SSZ_VAR_NODE_WORDS, 0xdeadbeefu);  // exact size: ASan sees a node out of range
  const SszVar v = ssz_var_shape(kind, obj_len, obj[obj_len - 1]);
  uint32_t dependent = 0;
  for (uint32_t ph = 0; ph < ssz_var_phases(v); ph++) {
    uint32_t busiest = 0;
    for (uint32_t lane = 0; lane < SSZ_VAR_LANES; lane++)
      busiest = std::max(busiest, ssz_var_step(v, ph, lane, obj, domain, nodes.data(), out));
    dependent += busiest;
  }
  return dependent;
}

// the issue's bound: sum over the levels of the chunk tree of ceil(pairs / 64), plus 15 for the
// containers (AttestationData 9, mix-in 1, Attestation 2, AggregateAndProof 2, SigningData 1)
static uint32_t bound(uint32_t kind, uint32_t n_bits) {
  uint32_t cnt = std::max((n_bits + 255) / 256, 1u), sum = 0;
  for (uint32_t l = 0; l < (kind == 2 ? 9u : 3u); l++) {
    const uint32_t pairs = (cnt + 1) / 2;
    sum += (pairs + 63) / 64;
    cnt = pairs;
  }
  return sum + 15;
}

static int run_roots(const char* in, const char* out) {
  FILE* fi = fopen(in, "r");
  FILE* fo = fopen(out, "w");
  if (!fi || !fo) return 2;
  static char a[40000], b[128];
  unsigned kind = 0;
  while (fscanf(fi, "%u %39000s %100s", &kind, a, b) == 3) {
    const std::vector<uint8_t> obj = unhex(a), dom = unhex(b);
    if (dom.size() != 32) return 3;
    // exact-size heap buffers: a read or a store past either end is an ASan report
    std::vector<uint8_t> o(obj), d(dom), r(32, 0xaa), payload(obj);
    payload.insert(payload.end(), dom.begin(), dom.end());
    const std::vector<uint8_t> before(payload);
    lsg_set t;
    memset(&t, 0, sizeof t);
    t.msg = payload.data();
    t.msg_len = LSG_MSG_OBJECT | (kind << LSG_MSG_KIND_SHIFT) | (uint32_t)payload.size();
    if (!lsgp::msg_set_ok(t)) return 4;  // the stager admits what the driver is given
    if (lsgp::msg_bytes(t.msg_len) != payload.size() || lsgp::msg_kind_tag(t.msg_len) != kind) return 5;
    uint32_t dep = 0, dep2 = 0, bnd = 0;
    if (kind == 0) {
      if (!ssz_object_signing_root((uint32_t)o.size(), o.data(), d.data(), r.data())) return 6;
      if (!ssz_object_signing_root((uint32_t)obj.size(), payload.data(), payload.data() + obj.size(), payload.data())) return 6;
      if (lsgp::msg_object_kind(t.msg_len) != obj.size()) return 7;
    } else {
      dep = var_root(kind, o.data(), (uint32_t)o.size(), d.data(), r.data());
      dep2 = var_root(kind, payload.data(), (uint32_t)obj.size(), payload.data() + obj.size(), payload.data());
      if (dep != dep2) return 8;
      bnd = bound(kind, ssz_var_shape(kind, (uint32_t)o.size(), o.back()).n_bits);
    }
    if (memcmp(payload.data() + 32, before.data() + 32, before.size() - 32)) return 9;  // only 32 bytes written
    fprintf(fo, "%s %s %u %u\n", hex(r.data(), 32).c_str(), hex(payload.data(), 32).c_str(), dep, bnd);
  }
  fclose(fi);
  fclose(fo);
  return 0;
}

static int run_zero() {
  for (int d = 0; d < 10; d++) {
    uint8_t b[32];
    ssz_store(b, SSZ_ZERO[d]);
    printf("%s\n", hex(b, 32).c_str());
  }
  return 0;
}

static int run_classify() {
  // "<tag> <len> | marked: bytes tag marked fixed kind | unmarked: bytes tag marked fixed kind"
  const uint32_t lens[] = {0, 32, 160, 296, 369, 0x00ffffffu};
  for (uint32_t tag = 0; tag < 128; tag++)
    for (uint32_t len : lens) {
      const uint32_t m = LSG_MSG_OBJECT | (tag << LSG_MSG_KIND_SHIFT) | len, u = (tag << LSG_MSG_KIND_SHIFT) | len;
      printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", tag, len, lsgp::msg_bytes(m), lsgp::msg_kind_tag(m),
             (unsigned)lsgp::msg_marked(m), (unsigned)lsgp::msg_fixed_object(m), lsgp::msg_object_kind(m), lsgp::msg_bytes(u),
             lsgp::msg_kind_tag(u), (unsigned)lsgp::msg_marked(u), (unsigned)lsgp::msg_fixed_object(u), lsgp::msg_object_kind(u));
    }
  return 0;
}

// a well-formed object of `nbytes` bitlist bytes whose last byte is `last`
static std::vector<uint8_t> make(uint32_t kind, uint32_t nbytes, uint8_t last) {
  const uint32_t off = kind == 2 ? 344 : 336;
  std::vector<uint8_t> o(off + nbytes, 0x5a);
  const uint32_t o1 = 108, o2 = off - 108;
  memcpy(o.data() + 8, &o1, 4);
  memcpy(o.data() + 108, &o2, 4);
  o.back() = last;
  return o;
}
static bool set_ok(uint32_t kind, const std::vector<uint8_t>& obj) {
  std::vector<uint8_t> payload(obj);  // exactly object + domain
  payload.resize(obj.size() + 32, 0x11);
  lsg_set t;
  memset(&t, 0, sizeof t);
  t.msg = payload.data();
  t.msg_len = LSG_MSG_OBJECT | (kind << LSG_MSG_KIND_SHIFT) | (uint32_t)payload.size();
  lsg_job job = {&t, 1, LSG_JOB_BATCHABLE};
  const bool ok = lsgp::msg_set_ok(t);
  if (ok != lsgp::msg_sets_ok(&t, 1) || ok != lsgp::msg_jobs_ok(&job, 1)) abort();
  if (kind && ok != lsgp::msg_var_ok(kind, obj.data(), obj.size())) abort();
  return ok;
}

static int run_args() {
  for (uint32_t kind = 1; kind <= 2; kind++) {
    const uint32_t maxb = kind == 2 ? 16385 : 257, off = kind == 2 ? 344 : 336;
    // the well-formed twins: the shortest, a middle one, the longest
    if (!set_ok(kind, make(kind, 1, 1)) || !set_ok(kind, make(kind, 1, 0x80)) || !set_ok(kind, make(kind, 33, 0x1f)) ||
        !set_ok(kind, make(kind, maxb, 1)) || !set_ok(kind, make(kind, maxb - 1, 0xff)))
      return 20;
    std::vector<uint8_t> o = make(kind, 33, 0x1f);
    o[8] ^= 1;  // the outer offset
    if (set_ok(kind, o)) return 21;
    o = make(kind, 33, 0x1f);
    o[108] ^= 8;  // the inner offset (the other kind's)
    if (set_ok(kind, o)) return 22;
    o = make(kind, 33, 0x1f);
    o[111] = 1;  // its high byte
    if (set_ok(kind, o)) return 22;
    if (set_ok(kind, make(kind, 33, 0)) || set_ok(kind, make(kind, 1, 0))) return 23;  // no delimiter bit
    if (set_ok(kind, make(kind, maxb, 2)) || set_ok(kind, make(kind, maxb, 0x80))) return 24;  // limit + 1 bits and more
    if (set_ok(kind, make(kind, maxb + 1, 1))) return 25;                                      // a byte too long
    std::vector<uint8_t> fixed_only(off, 0x5a), shorter(off - 1, 0x5a), tiny(4, 0);
    if (set_ok(kind, fixed_only) || set_ok(kind, shorter) || set_ok(kind, tiny)) return 26;  // no bitlist byte
    if (set_ok(kind == 1 ? 2 : 1, make(kind, 33, 0x1f))) return 27;  // the other tag: the inner offset differs
    // a payload of 32 bytes or fewer leaves no object
    uint8_t dom[32] = {0};
    lsg_set t;
    memset(&t, 0, sizeof t);
    t.msg = dom;
    for (uint32_t len = 0; len <= 32; len++) {
      t.msg_len = LSG_MSG_OBJECT | (kind << LSG_MSG_KIND_SHIFT) | len;
      if (lsgp::msg_set_ok(t)) return 28;
    }
    // msg == NULL
    t.msg = nullptr;
    t.msg_len = LSG_MSG_OBJECT | (kind << LSG_MSG_KIND_SHIFT) | (off + 33);
    if (lsgp::msg_set_ok(t)) return 29;
  }
  // unknown tags, over a buffer that would be well-formed under tag 1 and 2
  for (uint32_t tag = 3; tag < 128; tag++)
    if (set_ok(tag, make(1, 33, 0x1f)) || set_ok(tag, make(2, 33, 0x1f))) return 30;
  // tag 0 still goes by length; 296 is a kind, the tagged lengths are not
  std::vector<uint8_t> cap(264, 1);
  if (!set_ok(0, cap) || set_ok(0, make(1, 33, 0x1f))) return 31;
  // unmarked words are byte counts in all their bits, and pass
  uint8_t one = 0;
  lsg_set t;
  memset(&t, 0, sizeof t);
  t.msg = &one;
  for (uint32_t len : {0x01000000u, 0x01000171u, 0x7f000000u, 0x7fffffffu}) {
    t.msg_len = len;
    if (!lsgp::msg_set_ok(t) || lsgp::msg_bytes(len) != len || lsgp::msg_kind_tag(len) != 0) return 32;
  }
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "roots")) return run_roots(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "zero")) return run_zero();
  if (argc == 2 && !strcmp(argv[1], "classify")) return run_classify();
  if (argc == 2 && !strcmp(argv[1], "args")) return run_args();
  fprintf(stderr, "usage: sszvarcheck roots IN OUT | zero | classify | args\n");
  return 1;
}
