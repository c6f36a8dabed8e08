// CPU build (g++ -O1 -fsanitize=undefined -fno-sanitize-recover=undefined) of mul2 (fe29.cuh: (a b + c d) / R with one reduction)
// and of the group-law forms of ec29.cuh whose hot path uses it.  A stand-alone program: tests/test_fused_products_cpu.py runs it
// as a child process, writes one request per line to its standard input and reads one answer per line.  Any signed overflow in a
// 64-bit column sum aborts it, so a clean run over operands at the contract's bounds is the proof of the column bound.
// Test infrastructure only -- never linked into the product.
//   M <36 ints: raw limbs of a, b, c, d>      -> canonical (a b + c d) / R as 64 hex digits
//   E <27 ints: raw limbs of a, b, d>         -> canonical mul2(a, b, 0, d) and canonical mul(a, b)
//   P <op> <128 hex digits> <128 hex digits>  -> rc and the sum as a boundary point (op: tests/fused_product_cases.py)
#include <cstdio>
#include <cstring>
#include "../../mpc_bulletproof_amd/csrc/ec29.cuh"
using namespace bp;

static bool read_fp(Fp &x) {
  for (int j = 0; j < NL; j++)
    if (scanf("%d", &x.v[j]) != 1) return false;
  return true;
}
static void print_words(const uint32_t *w, int n) {
  for (int j = n - 1; j >= 0; j--) printf("%08x", w[j]);
}
static void print_canon(const Fp &x) {
  uint32_t w[8];
  pack(w, canon(x));
  print_words(w, 8);
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
static Jac rescale(const Jac &p, const uint32_t zw[8]) {   // (X z^2 : Y z^3 : Z z), the same point
  if (jac_is_inf(p)) return p;
  Fp z = to_mont(unpack<FP>(zw));
  Fp z2 = sqr(z), z3 = mul(z2, z);
  Jac r;
  r.X = mul(p.X, z2); r.Y = mul(p.Y, z3); r.Z = mul(p.Z, z);
  return r;
}
static int point_op(int op, const uint32_t wa[16], const uint32_t wb[16], uint32_t wo[16]) {
  Aff p, q;
  if (!aff_from_boundary(p, wa) || !aff_from_boundary(q, wb)) return -1;
  const uint32_t z1[8] = {0x12345, 7, 9, 0, 0, 0, 0, 0}, z2[8] = {0x54321, 11, 5, 0, 0, 0, 0, 0};
  Jac pj = jac_from_aff(p), r;
  switch (op) {
    case 0: r = jac_madd(pj, q); break;
    case 1: r = jac_add(rescale(pj, z2), rescale(jac_from_aff(q), z1)); break;
    case 3: r = xyzz_to_jac(xyzz_madd(xyzz_madd(xyzz_inf(), p), q)); break;
    case 4:
      if (aff_is_inf(q)) return -3;
      r = xyzz_to_jac(xyzz_madd_nzq(xyzz_from_jac(rescale(pj, z2)), q));
      break;
    case 5:
      if (aff_is_inf(q)) return -3;
      r = jac_madd_nzq(rescale(pj, z1), q);
      break;
    default: return -2;
  }
  aff_to_boundary(wo, jac_to_aff(r));
  return 0;
}

int main() {
  char cmd[8];
  while (scanf("%7s", cmd) == 1) {
    if (cmd[0] == 'M') {
      Fp a, b, c, d;
      if (!read_fp(a) || !read_fp(b) || !read_fp(c) || !read_fp(d)) return 2;
      print_canon(mul2(a, b, c, d));
      printf("\n");
    } else if (cmd[0] == 'E') {
      Fp a, b, d;
      if (!read_fp(a) || !read_fp(b) || !read_fp(d)) return 2;
      print_canon(mul2(a, b, fe_zero<FP>(), d));
      printf(" ");
      print_canon(mul(a, b));
      printf("\n");
    } else if (cmd[0] == 'P') {
      int op;
      uint32_t wa[16], wb[16], wo[16];
      if (scanf("%d", &op) != 1 || !read_point_bytes(wa) || !read_point_bytes(wb)) return 2;
      memset(wo, 0, sizeof wo);
      const int rc = point_op(op, wa, wb, wo);
      printf("%d ", rc);
      for (int i = 0; i < 64; i++) printf("%02x", ((const uint8_t *)wo)[i]);
      printf("\n");
    } else return 2;
  }
  return 0;
}
