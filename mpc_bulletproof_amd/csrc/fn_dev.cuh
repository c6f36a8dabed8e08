// fn_dev.cuh -- device helpers for F_n kernels shared by k_scalar.hip and the fused verification launches of k_ec.hip.
#pragma once
#include "fe29.cuh"
#include "kernels.h"

namespace bpk {
using namespace bp;

BP_HD Fn load_words(const Words8 *p) {   // 8 words as they stand (a Montgomery coefficient, ark limbs) -> limbs
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = p->w[j];
  return unpack<FN>(w);
}
BP_HD Fn load_plain(const Words8 *p) { return to_mont(load_words(p)); }   // plain canonical words -> Montgomery
BP_HD bool words_canonical(const Words8 *p) {   // the 8 words are below n
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = p->w[j];
  return words_lt_mod<FN>(w);
}
__device__ __forceinline__ void store_plain(Words8 *p, const Fn &x) {   // Montgomery -> plain canonical words
  uint32_t w[8];
  pack(w, from_mont(x));
#pragma unroll
  for (int j = 0; j < 8; j++) p->w[j] = w[j];
}
__device__ __forceinline__ Fn fn_from_u32(uint32_t v) {
  Fn t = fe_zero<FN>();
  t.v[0] = (int32_t)(v & LMASK);
  t.v[1] = (int32_t)(v >> LB);
  return to_mont(t);
}
BP_HD Fn fn_pow_u32(Fn base, uint32_t e) {   // base^e, e >= 0
  Fn acc = fe_one<FN>();
  while (e) {
    if (e & 1) acc = mul(acc, base);
    e >>= 1;
    if (e) base = sqr(base);
  }
  return acc;
}
// Lazy sums keep limbs small but let the VALUE grow (top limb has ~11 spare bits over a 252-bit
// modulus): fold the value back into (-eps, (1+eps) n) with one Montgomery multiplication by R mod n.
// Rule used below: fold every 4, 8 or 16 loop trips (at most 33 lazy terms), once more before a wave_sum, and end the 4-wave add
// (256 reduced values) with store_plain or fn_reduce.  Measured headroom (tests/test_lazy_sums_cpu.py, heaviest terms -- lazy value
// n - 1 -- on a UBSan build): 4095 unreduced products may be added before fn_reduce and 4095 reduced values before the last
// reduction; the 4096th wraps the top limb (4096 * 2^19 = 2^31).  The values then are far past the |v| < 2^256 that mul documents for
// two general operands: fn_reduce's other operand is R mod n < n, which is what leaves the room.
// The verifier's sites against that headroom (tests/verifier_sum_cases.py drives each across its fold): flatten_column below 1 + 16
// products, and its callers add at most two more products to the lazy column; the delta and `One`-column loops of
// k_verify_scalars(_fast) and k_vsl_gh / k_vsl_wc 1 + 16 products per lane, then 64 reduced lanes (2 reduced waves per block of the
// grid-split route); k_vsl_tail 1 + 8 partials of 2 reduced values each; k_sc_weighted_colsum, comb_colsum_body (k_pip2.hip) and
// mix_colsum_body (k_mixed.hip) 1 + 16 products per lane, then 256 reduced values.
BP_HD Fn fn_reduce(const Fn &x) { return mul(x, fe_one<FN>()); }
// raw limb I/O for device scratch (zpow tables, partial sums)
__device__ __forceinline__ void raw_put(int32_t *d, const Fn &x) {
#pragma unroll
  for (int j = 0; j < NL; j++) d[j] = x.v[j];
}
__device__ __forceinline__ Fn raw_get(const int32_t *s) {
  Fn x;
#pragma unroll
  for (int j = 0; j < NL; j++) x.v[j] = s[j];
  return x;
}
// wave-level sum of one Fn per lane (shuffle tree); result in every lane
#if defined(__HIPCC__)
__device__ __forceinline__ Fn wave_sum(Fn x) {
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    Fn o;
#pragma unroll
    for (int j = 0; j < NL; j++) o.v[j] = __shfl_xor(x.v[j], off, 64);
    x = add(x, o);
  }
  return x;
}
// the block tail of every sum: one lazy Fn per lane over a block of TPB lanes -- fn_reduce, wave_sum, the waves' sums (64 reduced values
// each) through one LDS slot each and added by thread 0, which alone holds the result; it ends the sum with store_plain or fn_reduce.
// Every thread of the block calls it; the closing barrier frees the slots for another call.
template <int TPB> __device__ __forceinline__ Fn block_sum(Fn acc) {
  static_assert(TPB % 64 == 0, "whole waves");
  acc = wave_sum(fn_reduce(acc));
  if constexpr (TPB > 64) {
    __shared__ int32_t sm[NL * (TPB / 64)];
    if ((threadIdx.x & 63) == 0) raw_put(sm + (threadIdx.x >> 6) * NL, acc);
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < TPB / 64; w++) acc = add(acc, raw_get(sm + w * NL));
    __syncthreads();
  }
  return acc;
}
#endif

// one flattened constraint weight: output o of the column-major circuit against a proof's z-power table (flattened_constraints,
// prover.rs:342-379; w_V and w_c carry the reference's minus sign)
__device__ __forceinline__ Fn flatten_column(const CircuitDev &c, size_t o, const int32_t *zp) {
  Fn acc = fe_zero<FN>();
  uint32_t cnt = 0;
  for (uint32_t t = c.col_ptr[o]; t < c.col_ptr[o + 1]; t++) {
    acc = add(acc, mul(load_words(&c.coeff[t]), raw_get(zp + (size_t)c.row[t] * NL)));
    if ((++cnt & 15) == 0) acc = fn_reduce(acc);
  }
  if (o >= 3 * c.n) acc = neg(acc);
  return acc;
}
// one constraint row of the row-major view against one prover's witness (Prover::constraints_satisfied, prover.rs:405-409, and a
// party's local half of mpc_prover.rs:556-568): the terms lo, lo + step, .. below hi of sum coeff * chi_j * value.  The values are
// the prover's plain canonical planes; `one` is what a `One` term reads (1, or 0 on a share or MAC plane); chi: the prover's
// gadget challenges (plain canonical words; never read when no term has j > 0).  The stored coefficients carry no sign: the minus
// of w_V and w_c is flatten_column's.  Lazy like flatten_column: the caller reduces the result (fn_reduce) before it sums further.
BP_HD Fn eval_row(const RowsDev &rv, uint32_t lo, uint32_t hi, uint32_t step, const Words8 *aL, const Words8 *aR, const Words8 *aO,
                  const Words8 *v, const Fn &one, const Words8 *chi) {
  Fn acc = fe_zero<FN>();
  uint32_t cnt = 0;
  for (uint32_t t = lo; t < hi; t += step) {
    Fn cf = load_words(&rv.coeff[t]);
    const uint32_t code = rv.var[t], j = code >> ROWS_CHI_SHIFT, kind = (code >> ROWS_KIND_SHIFT) & 7u, idx = code & ROWS_IDX_MASK;
    if (j) cf = mul(cf, load_plain(chi + (j - 1)));
    const Words8 *pl = kind == 0 ? aL : (kind == 1 ? aR : (kind == 2 ? aO : v));
    acc = add(acc, mul(cf, kind == 4 ? one : load_plain(pl + idx)));
    if ((++cnt & 15) == 0) acc = fn_reduce(acc);
  }
  return acc;
}

}  // namespace bpk
