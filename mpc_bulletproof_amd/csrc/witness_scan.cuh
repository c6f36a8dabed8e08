// witness_scan.cuh -- the product chains of a bpgpu_witness program as a segmented prefix product: what every thread of k_witness_scan
// (k_witness.hip) runs on its own run of chain members, and what tests/csrc/witness_scan_host_test.cpp compiles for the CPU.  Below
// the product pieces, the same for chains with affine members as a segmented prefix composition of affine maps (wit_aff_*,
// tests/csrc/witness_affine_host_test.cpp).
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

// ---- affine chains: the same scan over the monoid of affine maps -----------------------------------------------------------------------
// An AFFINE member e (WIT_ELEM_AFFINE) has the link row c_e a_O[pred] + f_e and the free row g_e, f_e and g_e reading nothing of their
// phase: a_O[e] = A_e a_O[pred] + B_e with A_e = c_e g_e, B_e = f_e g_e.  A product member is the map with f = 0.  The maps compose
// associatively, (A2, B2) o (A1, B1) = (A2 A1, A2 B1 + B2), and F_n arithmetic on canonical values is exact: any bracketing stores
// the bytes of the gates one by one.  The link term stands first in the library's copy of the link row, so wit_link reads it as it
// reads a product member's; f is eval_row over the rest of the row.  A chain's FIRST member becomes the constant map
// x -> A a_O[head] + B, stored as (0, A a_O[head] + B): the b of whatever composition reaches a run is then a_O of the element before it.
struct WitAff { Fn a, b; uint32_t flag; };

BP_HD WitAff wit_aff_identity() { return {fe_one<FN>(), fe_zero<FN>(), 0u}; }
// The segmented operator: `x` the earlier run, `y` the later one; y alone where y starts a segment.  The two products are independent.
// Limb bound: every `a` is zero, one or a mul output, and so is x.a.  A `b` is a SUM, counted here in mul outputs (each tight, within
// one modulus n < 2^252 of zero; add() normalises to T'): a member's map has b of 1 (f g), a first member's of 2; the fold of a run
// (wit_aff_local: y a member's map) gives 1 + 2 = 3; each of the 6 shuffle steps adds one product to the later part's b, 9 at the
// most; a wave's total folded into the carry, and the carry into the lanes below, give 1 + 9 = 10.  The count depends on the shape of
// the scan, not on the chain's length, and 10 n < 2^256: x.b stays inside what mul asks (|v| < 2^256, T') without a reduction.
BP_HD WitAff wit_aff_combine(const WitAff &x, const WitAff &y) {
  const Fn a = mul(y.a, x.a), b = add(mul(y.a, x.b), y.b);
  WitAff r;
#pragma unroll
  for (int j = 0; j < NL; j++) {
    r.a.v[j] = y.flag ? y.a.v[j] : a.v[j];
    r.b.v[j] = y.flag ? y.b.v[j] : b.v[j];
  }
  r.flag = x.flag | y.flag;
  return r;
}
// the rest of member i's link row, after its first term
BP_HD Fn wit_aff_rest(const WitDev &w, uint32_t i, bool right, const WitPlanes &o) {
  const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
  return fn_reduce(eval_row(w.rows, (right ? rp[1] : rp[0]) + 1, right ? rp[2] : rp[1], 1, o.aL, o.aR, o.aO, o.v, fe_one<FN>(), o.chi));
}
// First pass over the elements [lo, hi): g is stored on the free side (it is final), f of an affine member is parked in its link-side
// slot (nobody reads that slot before the second pass: the gates that do sit on later levels), and the run's map comes back.
BP_HD WitAff wit_aff_local(const WitDev &w, uint32_t lo, uint32_t hi, const WitPlanes &o) {
  WitAff p = wit_aff_identity();
  const Fn one = fe_one<FN>();
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t word = w.chain_elem[e], i = word & ROWS_IDX_MASK;
    const bool right = (word & WIT_ELEM_RIGHT) != 0;
    const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
    const Fn g = fn_reduce(eval_row(w.rows, right ? rp[0] : rp[1], right ? rp[1] : rp[2], 1, o.aL, o.aR, o.aO, o.v, one, o.chi));
    wit_store((right ? o.aL : o.aR) + i, g);
    const WitLink k = wit_link(w, word, o.chi);
    WitAff m{mul(k.c, g), fe_zero<FN>(), word & WIT_ELEM_START};
    if (word & WIT_ELEM_AFFINE) {
      const Fn f = wit_aff_rest(w, i, right, o);
      wit_store((right ? o.aR : o.aL) + i, f);
      m.b = mul(f, g);
    }
    if (m.flag) {
      m.b = add(mul(m.a, load_plain(o.aO + k.pred)), m.b);
      m.a = fe_zero<FN>();
    }
    p = wit_aff_combine(p, m);
  }
  return p;
}
// Second pass: `carry` is a_O of the element before the run (the b of the composition of the parts before it; up to 10 mul outputs,
// see wit_aff_combine).  Only the head's a_O (from before the barrier) and what this thread stored in the first pass is read.
BP_HD void wit_aff_apply(const WitDev &w, uint32_t lo, uint32_t hi, const Fn &carry, const WitPlanes &o) {
  Fn prev = carry;
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t word = w.chain_elem[e], i = word & ROWS_IDX_MASK;
    const bool right = (word & WIT_ELEM_RIGHT) != 0;
    const WitLink k = wit_link(w, word, o.chi);
    if (word & WIT_ELEM_START) prev = load_plain(o.aO + k.pred);
    Fn link = mul(k.c, prev);
    if (word & WIT_ELEM_AFFINE) link = add(link, load_plain((right ? o.aR : o.aL) + i));     // the parked f
    prev = mul(link, load_plain((right ? o.aL : o.aR) + i));
    wit_store((right ? o.aR : o.aL) + i, link);
    wit_store(o.aO + i, prev);
  }
}

}  // namespace bpk
