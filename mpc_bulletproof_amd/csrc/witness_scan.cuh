// witness_scan.cuh -- the product chains of a bpgpu_witness program as a segmented prefix product: what every thread of k_witness_scan
// (k_witness.hip) runs on its own run of chain members, and what tests/csrc/witness_scan_host_test.cpp compiles for the CPU.
//
// A chain is head -> member -> member ..: member e is multiply(c_e a_O[pred], free row) with the link on either side, so
// a_O[e] = a_O[head] * prod_{k <= e} f_k, f_k = c_k r_k, r_k = eval(free row of k).  The factors read nothing of their own phase, F_n
// multiplication is exactly associative on canonical values, and every stored value is canonical: any bracketing gives the bytes of the
// gate-by-gate evaluation.  No inversion anywhere: a zero factor zeroes the products after it, as it does gate by gate.
//
// Limb bound: every operand of mul here is a mul output (load_plain, fn_reduce and the products themselves: tight limbs, value within
// one modulus of zero) or the unpacked canonical coefficient of the handle (tight, < n) -- both inside |v| < 2^256 and T' that mul asks
// of two general operands (fe29.cuh), so products feed products for any chain length without a reduction in between.
#pragma once
#include "witness_dev.cuh"

namespace bpk {

// the scanned value of a run of elements: the product since the run's last segment start (or of the whole run), and whether it has one
struct WitPart { Fn v; uint32_t flag; };

BP_HD WitPart wit_part_identity() { return {fe_one<FN>(), 0u}; }
// the segmented operator: `a` the earlier run, `b` the later one.  Associative; b's value alone where b starts a segment.
BP_HD WitPart wit_part_combine(const WitPart &a, const WitPart &b) {
  const Fn both = mul(a.v, b.v);
  WitPart r;
#pragma unroll
  for (int j = 0; j < NL; j++) r.v.v[j] = b.flag ? b.v.v[j] : both.v[j];
  r.flag = a.flag | b.flag;
  return r;
}

// what one prover's planes are to a thread
struct WitPlanes { Words8 *aL, *aR, *aO; const Words8 *v, *chi; };

// the link term of member `word` (its only term): the coefficient on the prover's challenges, and the gate it reads
struct WitLink { Fn c; uint32_t pred; };
BP_HD WitLink wit_link(const WitDev &w, uint32_t word, const Words8 *chi) {
  const uint32_t i = word & ROWS_IDX_MASK, t = w.rows.row_ptr[2 * (size_t)i + ((word & WIT_ELEM_RIGHT) ? 1 : 0)];
  uint32_t cw[8];
#pragma unroll
  for (int j = 0; j < 8; j++) cw[j] = w.rows.coeff[t].w[j];
  WitLink k{unpack<FN>(cw), w.rows.var[t] & ROWS_IDX_MASK};
  const uint32_t j = w.rows.var[t] >> ROWS_CHI_SHIFT;
  if (j) k.c = mul(k.c, load_plain(chi + (j - 1)));
  return k;
}

// First pass over the elements [lo, hi) of chain_elem: the free side of every member is stored (it is final), and the run's part
// comes back -- the first member of a chain carries its head's a_O, which the level's ordinary gates stored before the barrier.
BP_HD WitPart wit_scan_local(const WitDev &w, uint32_t lo, uint32_t hi, const WitPlanes &o) {
  WitPart p = wit_part_identity();
  const Fn one = fe_one<FN>();
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t word = w.chain_elem[e], i = word & ROWS_IDX_MASK;
    const bool right = (word & WIT_ELEM_RIGHT) != 0;
    const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
    const Fn r = fn_reduce(eval_row(w.rows, right ? rp[0] : rp[1], right ? rp[1] : rp[2], 1, o.aL, o.aR, o.aO, o.v, one, o.chi));
    wit_store((right ? o.aL : o.aR) + i, r);
    const WitLink k = wit_link(w, word, o.chi);
    WitPart f{mul(k.c, r), word & WIT_ELEM_START};
    if (f.flag) f.v = mul(f.v, load_plain(o.aO + k.pred));
    p = wit_part_combine(p, f);
  }
  return p;
}

// Second pass: `carry` is the product that reaches the run (the scan of the parts before it).  a_O[pred] of every element is the
// carry times the run's own prefix, so nothing another thread stored during the scan is read: only the head's a_O (from before the
// barrier) and the free side this thread stored in the first pass.
BP_HD void wit_scan_apply(const WitDev &w, uint32_t lo, uint32_t hi, const Fn &carry, const WitPlanes &o) {
  Fn prev = carry;
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t word = w.chain_elem[e], i = word & ROWS_IDX_MASK;
    const bool right = (word & WIT_ELEM_RIGHT) != 0;
    const WitLink k = wit_link(w, word, o.chi);
    if (word & WIT_ELEM_START) prev = load_plain(o.aO + k.pred);
    const Fn link = mul(k.c, prev);
    prev = mul(link, load_plain((right ? o.aL : o.aR) + i));
    wit_store((right ? o.aR : o.aL) + i, link);
    wit_store(o.aO + i, prev);
  }
}

}  // namespace bpk
