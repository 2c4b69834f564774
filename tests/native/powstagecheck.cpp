// TEST INFRASTRUCTURE ONLY -- stand-alone host driver of the stages that the signature decode
// and the SSWU map are cut into around their two powers (lsg_tower.hpp fp2_sqrt_root_c /
// fp2_sqrt_root_finish, lsg_curve.hpp g2_uncompress_parse / g2_uncompress_finish, lsg_h2c.hpp
// sswu_stage_a / b / c), composed the way the stage kernels compose them -- each power run by
// the one-element-per-lane lanes_pow_plan, not by the pair form -- beside the unsplit functions
// (g2_uncompress, map_to_curve_sswu_ni).  One-lane host build of the pair backend.
//
//   powstagecheck IN OUT
// IN: one item per line: "S" and 192 hex digits (a 96-byte signature) or "M" and 192 hex digits
// (a field element u of Fp2: c0, c1 as 48 big-endian bytes each).  OUT per item: S: the code,
// the infinity flag and the 192-byte point (hex); M: the mapped point of E2' (192 bytes, hex).
// The driver compares the staged and the unsplit results limb for limb (and the codes) and exits
// with status 1 at the first difference.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LSG_PAIR_G 1
#include "lsg_fp_pair.hpp"
#include "lsg_h2c.hpp"

// a power as k_fp_pow_lanes computes it
static fp_t lane_pow(const fp_t& a, int id) {
  fpl_t x;
  for (int k = 0; k < 14; k++) x.l[k] = a.l[k];
  const fpl_t r = lanes_pow_plan(x, id);
  fp_t o;
  for (int k = 0; k < 14; k++) o.l[k] = r.l[k];
  return o;
}
static bool same(const fp2_t& a, const fp2_t& b) { return memcmp(&a, &b, sizeof a) == 0; }

// k_sig_decode_a / b / c on one item
static int staged_uncompress(g2a_t& out, bool& inf, const uint8_t* in) {
  fp2_t x, rhs;
  bool want = false;
  const int e = g2_uncompress_parse(out, inf, x, rhs, want, in);
  if (e != LSG_UNCOMPRESS_PENDING) return e;
  const fp_t n = fp2_norm(rhs);
  const fp_t cand = lane_pow(n, LSG_POW_SQRT);
  const bool ok = fp_is_root_of(cand, n);
  const fp_t c = fp2_sqrt_root_c(rhs, cand);
  const fp_t t = lane_pow(c, LSG_POW_SQRT34);
  fp2_t y;
  const bool root = fp2_sqrt_root_finish(y, rhs, c, t);
  return g2_uncompress_finish(out, x, y, ok && root, want);
}
// k_h2c_map_a / b / c on one item (before the isogeny)
static g2a_t staged_sswu(const fp2_t& u, const fp_t& ni) {
  sswu_mid_t m = sswu_stage_a(u, ni);
  const fp_t n = fp2_norm(m.gx1);
  const fp_t s1 = lane_pow(n, LSG_POW_SQRT);
  fp2_t x, gx;
  const fp_t c = sswu_stage_b(x, gx, m, u, n, s1);
  const fp_t t = lane_pow(c, LSG_POW_SQRT34);
  return sswu_stage_c(u, x, gx, c, t);
}

static int hexval(int c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
static void puthex(FILE* f, const uint8_t* b, int n) {
  for (int i = 0; i < n; i++) fprintf(f, "%02x", b[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: powstagecheck IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) {
    fprintf(stderr, "powstagecheck: cannot open files\n");
    return 2;
  }
  char kind[4], hex[256];
  long item = 0;
  for (; fscanf(in, "%3s %200s", kind, hex) == 2; item++) {
    if (strlen(hex) != 192) {
      fprintf(stderr, "powstagecheck: item %ld: %zu hex digits\n", item, strlen(hex));
      return 2;
    }
    uint8_t b[96], o[192];
    for (int i = 0; i < 96; i++) b[i] = (uint8_t)(hexval(hex[2 * i]) << 4 | hexval(hex[2 * i + 1]));
    g2a_t p, q;
    p.x = p.y = q.x = q.y = fp2_zero();
    if (kind[0] == 'S') {
      bool pinf = false, qinf = false;
      const int e = staged_uncompress(p, pinf, b), f = g2_uncompress(q, qinf, b);
      if (e != f || pinf != qinf || !same(p.x, q.x) || !same(p.y, q.y)) {
        fprintf(stderr, "powstagecheck: item %ld: staged decode (%d) differs from g2_uncompress (%d)\n", item, e, f);
        return 1;
      }
      g2_serialize(o, p, pinf);
      fprintf(out, "%d %d ", e, pinf ? 1 : 0);
    } else {
      const fp2_t u = fp2_make(fp_to_mont(fp_from_be48(b)), fp_to_mont(fp_from_be48(b + 48)));
      const fp_t ni = fp_inv(fp2_norm(sswu_tv1(u)));
      p = staged_sswu(u, ni);
      q = map_to_curve_sswu_ni(u, ni);
      if (!same(p.x, q.x) || !same(p.y, q.y)) {
        fprintf(stderr, "powstagecheck: item %ld: staged map differs from map_to_curve_sswu_ni\n", item);
        return 1;
      }
      g2_serialize(o, p, false);
    }
    puthex(out, o, 192);
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld\n", item);
  return 0;
}
