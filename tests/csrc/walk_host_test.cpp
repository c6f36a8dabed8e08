// CPU build (g++ -O1 -fsanitize=undefined -fno-sanitize-recover=undefined) of the accumulator walk of the table kernels: an
// extended-Jacobian accumulator that starts as xyzz_inf() and takes a list of affine addends, each with a digit's sign applied limb
// by limb (fp_sign_nr), through xyzz_madd_nzq -- the identity resolved through the one-limb filter, cancellations and doublings
// through the out-of-line complete addition.  A stand-alone program: tests/test_walk_identity_cpu.py runs it as a child process, one
// request per line on its standard input, one answer per line.  Test infrastructure only -- never linked into the product.
//   W <k> <d_1> <128 hex digits> ... <d_k> <128 hex digits>   -> the accumulator after every addend as a boundary point, then the
//                                                                 count of products that took an operand negated limb by limb
// After every addition the four stored coordinates must be T / T' (fe29.cuh), and every operand of every product of the group law
// must be inside its contract (the hook BP_FP_OPERANDS of ec29.cuh); a violation ends the program with status 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>

namespace chk {
constexpr int64_t B = (1ll << 29) + 8;          // the largest magnitude of a lower limb of T', and of a mul2 operand
constexpr int64_t WIDE = 3ll << 28;             // 1.5 * 2^29: what mul takes against a T' operand
constexpr int64_t TOP = 1ll << 24;              // |value| < 2^256 with lower limbs below 2^30: the top limb stays below 2^24
static long negated_operands = 0;
static void fail(const char *what) {
  fprintf(stderr, "contract violated: %s\n", what);
  exit(3);
}
template <class T> static int64_t lower_max(const T &x) {
  int64_t m = 0;
  for (int j = 0; j < 8; j++) { int64_t a = x.v[j] < 0 ? -(int64_t)x.v[j] : x.v[j]; if (a > m) m = a; }
  return m;
}
template <class T> static bool all_nonpositive(const T &x) {
  bool some = false;
  for (int j = 0; j < 8; j++) { if (x.v[j] > 8) return false; if (x.v[j] < -8) some = true; }
  return some;
}
template <class T> static void top_ok(const T &x) {
  if (x.v[8] >= TOP || x.v[8] <= -TOP) fail("|value| >= 2^256");
}
template <class T> static void operands(int k, const T &a, const T &b, const T &c, const T &d) {
  top_ok(a); top_ok(b);
  if (all_nonpositive(a) || all_nonpositive(b)) negated_operands++;
  if (k == 4) {
    top_ok(c); top_ok(d);
    if (lower_max(a) > B || lower_max(b) > B || lower_max(c) > B || lower_max(d) > B) fail("mul2 operand above 2^29 + 8");
    return;
  }
  const int64_t ma = lower_max(a), mb = lower_max(b);
  if (ma > WIDE || mb > WIDE) fail("mul operand above 1.5 * 2^29");
  if (ma > B && mb > B) fail("mul: neither operand within T'");
}
}  // namespace chk
#define BP_FP_OPERANDS(k, a, b, c, d) chk::operands(k, a, b, c, d)
#include "../../mpc_bulletproof_amd/csrc/ec29.cuh"
using namespace bp;

static void stored(const Fp &x, const char *name) {      // T / T': lower limbs in [-8, 2^29 + 8), the value below 2^256
  for (int j = 0; j < 8; j++)
    if (x.v[j] < -8 || x.v[j] >= (1 << 29) + 8) { fprintf(stderr, "stored %s limb %d = %d\n", name, j, x.v[j]); exit(3); }
  chk::top_ok(x);
}
static bool read_point_bytes(uint32_t w[16]) {
  char hex[129];
  if (scanf("%128s", hex) != 1 || strlen(hex) != 128) return false;
  uint8_t b[64];
  for (int i = 0; i < 64; i++) {
    unsigned v;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
    b[i] = (uint8_t)v;
  }
  memcpy(w, b, 64);
  return true;
}

int main() {
  char cmd[8];
  while (scanf("%7s", cmd) == 1) {
    if (cmd[0] != 'W') return 2;
    int k;
    if (scanf("%d", &k) != 1 || k < 0) return 2;
    Xyzz acc = xyzz_inf();
    if (!is_zero_limbs(acc.X) || !xyzz_is_inf(acc)) return 4;
    chk::negated_operands = 0;
    for (int i = 0; i < k; i++) {
      int d;
      uint32_t w[16], wo[16];
      if (scanf("%d", &d) != 1 || d == 0 || !read_point_bytes(w)) return 2;
      Aff q;
      if (!aff_from_boundary(q, w) || aff_is_inf(q)) return 5;
      const Fp y0 = q.y;
      q.y = fp_sign_nr(q.y, d);
      for (int j = 0; j < NL; j++)
        if (q.y.v[j] != (d < 0 ? -y0.v[j] : y0.v[j])) return 6;      // limb by limb, magnitudes unchanged
      acc = xyzz_madd_nzq(acc, q);
      stored(acc.X, "X"); stored(acc.Y, "Y"); stored(acc.ZZ, "ZZ"); stored(acc.ZZZ, "ZZZ");
      if (xyzz_is_inf(acc) && !is_zero_limbs(acc.X)) return 7;      // an identity that the walk made keeps the zero X
      Jac j = xyzz_to_jac(acc);
      if (!jac_is_inf(j) && is_zero_exact(j.Z)) return 8;            // Z = 0 (mod p) in a non-zero representation: no producer may leave one
      aff_to_boundary(wo, jac_to_aff(j));
      for (int t = 0; t < 64; t++) printf("%02x", ((const uint8_t *)wo)[t]);
      printf(" ");
    }
    printf("%ld\n", chk::negated_operands);
  }
  return 0;
}
