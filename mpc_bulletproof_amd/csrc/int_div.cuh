// int_div.cuh -- the integer quotient and remainder of two 256-bit integers held as 8 x 32-bit words, least significant first: the
// arithmetic of a BPGPU_GATE_DIVREM gate (witness_dev.cuh).  Plain C++ for the GPU and the CPU alike (tests/csrc/
// witness_divrem_host_test.cpp compiles it with g++); no inline assembly, and no dynamic index into the word arrays: every loop
// over words is unrolled with constant indices, so the operands stay in registers (a dynamic index becomes scratch memory).
//
// Restoring shift-and-subtract, bounded by the operands' bit lengths: with s = bitlen(x) - bitlen(y), the divisor is aligned under
// the dividend's top bit once (d = y << s, a barrel shift by words and then by bits) and s + 1 steps follow, each a conditional
// subtraction r -= d, a quotient bit shifted in, and d >>= 1.  A dividend below the divisor takes no step.  The result is a function
// of the two operands alone; lanes of a wave take the trip counts of their own operands.
#pragma once
#include <stdint.h>
#include "fe29.cuh"      // BP_HD

namespace bpk {

// the number of bits of the integer: 0 for zero, 256 at most
BP_HD uint32_t int_bitlen(const uint32_t (&w)[8]) {
  uint32_t top = 0, at = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    at = w[j] ? j : at;
    top = w[j] ? w[j] : top;
  }
  return top ? 32 * at + 32 - (uint32_t)__builtin_clz(top) : 0;
}
// w <<= s for s < 256; the caller knows that no set bit leaves the 256
BP_HD void int_shl(uint32_t (&w)[8], uint32_t s) {
  const uint32_t words = s >> 5, bits = s & 31;
#pragma unroll
  for (uint32_t step = 4; step; step >>= 1) {        // the word shift, one binary digit of it at a time
    const bool take = (words & step) != 0;
#pragma unroll
    for (uint32_t j = 8; j-- > 0;) {
      const uint32_t from = j >= step ? w[j - step] : 0;
      w[j] = take ? from : w[j];
    }
  }
#pragma unroll
  for (uint32_t j = 8; j-- > 0;) {                   // (32 - bits is 1 .. 32: in range for a 64-bit shift)
    const uint64_t two = ((uint64_t)w[j] << 32) | (j ? w[j - 1] : 0u);
    w[j] = (uint32_t)(two >> (32 - bits));
  }
}
// q = floor(x / y), r = x mod y; for y == 0: q = 0, r = x.  x = q y + r over the integers in either case.
BP_HD void int_divrem(uint32_t (&q)[8], uint32_t (&r)[8], const uint32_t (&x)[8], const uint32_t (&y)[8]) {
  uint32_t d[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { q[j] = 0; r[j] = x[j]; d[j] = y[j]; }
  const uint32_t bx = int_bitlen(x), by = int_bitlen(y);
  if (by == 0 || bx < by) return;
  const uint32_t s = bx - by;
  int_shl(d, s);                                     // bitlen(d) = bx <= 256
  for (uint32_t k = 0; k <= s; k++) {
    uint32_t t[8];
    bool borrow = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {                    // t = r - d, the borrow through the words (one subtract-with-borrow each on the GPU)
      uint32_t u;
      const bool b1 = __builtin_sub_overflow(r[j], d[j], &u), b2 = __builtin_sub_overflow(u, (uint32_t)borrow, &t[j]);
      borrow = b1 | b2;
    }
    const bool fits = !borrow;                       // r >= d
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = fits ? t[j] : r[j];
#pragma unroll
    for (int j = 8; j-- > 0;) q[j] = (q[j] << 1) | (j ? q[j - 1] >> 31 : (uint32_t)fits);
#pragma unroll
    for (int j = 0; j < 8; j++) d[j] = (d[j] >> 1) | (j < 7 ? d[j + 1] << 31 : 0u);
  }
}

}  // namespace bpk
