// mpc_witness_dev.cuh -- one gate of a bpgpu_witness program on ONE plane of an authenticated share (MpcProver::multiply /
// allocate_multiplier, r1cs_mpc/mpc_prover.rs:183-282): what every lane of k_mpc_witness.hip runs, and what
// tests/csrc/mpc_witness_host_test.cpp compiles for the CPU.  A virtual prover v = 3 p + k is plane k (0 share, 1 MAC, 2 public
// modifier) of proof p (k_mpc.hip).  The rows are eval_row's (fn_dev.cuh) with `one` = 1 on the modifier plane and 0 on the other
// two: a public constant is added to the modifier only, a public coefficient (c0 + sum chi_j c_j) scales all three planes alike.  The
// product of the two rows is not local: the gate's a_L, a_R are masked with a Beaver triple, and once the host has opened d and e the
// gate's a_O comes from beaver_term -- stated here once, for the polynomial build and the IPP rounds of k_mpc.hip as well.
#pragma once
#include "witness_dev.cuh"

namespace bpk {

// plane k of the Beaver product j of proof p at element i: z_k + d y_k + e x_k, plus d e on the modifier plane.  Layouts (plain
// canonical words): opened [p][j][d, e][i], trip [p][j][x, y, z][k][i], with nprod products per proof and len elements each
BP_HD Fn beaver_term(const Words8 *opened, const Words8 *trip, size_t p, size_t nprod, size_t j, int k, size_t len, size_t i) {
  const Words8 *o = opened + ((p * nprod + j) * 2) * len + i;
  const Words8 *t = trip + ((p * nprod + j) * 9 + k) * len + i;   // x at t, y at t + 3 len, z at t + 6 len
  const Fn d = load_plain(o), e = load_plain(o + len);
  Fn r = add(load_plain(t + 6 * len), add(mul(d, load_plain(t + 3 * len)), mul(e, load_plain(t))));
  if (k == 2) r = add(r, mul(d, e));
  return r;
}

// what one virtual prover reads and writes: its planes of n multipliers, of m committed values and of the input pairs (plain
// canonical words); chi: its PROOF's gadget challenges (public; never read when no term has j > 0)
struct MpcWitPlanes { Words8 *aL, *aR, *aO; const Words8 *v, *inputs, *chi; };
struct MpcWitPair { Fn L, R; };

BP_HD Fn mpc_wit_one(int k) { return k == 2 ? fe_one<FN>() : fe_zero<FN>(); }   // what a `One` term reads on plane k
// a_L, a_R of a gate on one plane from the lazy sums of its two rows; an INPUT gate takes the planes of its pair (arg)
BP_HD MpcWitPair mpc_wit_pair(uint32_t op, uint32_t arg, const Fn &left, const Fn &right, const Words8 *inputs) {
  if (op == WIT_OP_INPUT) return {load_plain(inputs + 2 * (size_t)arg), load_plain(inputs + 2 * (size_t)arg + 1)};
  return {fn_reduce(left), fn_reduce(right)};
}
// gate i on plane k, both rows by this lane
BP_HD MpcWitPair mpc_wit_rows(const WitDev &w, uint32_t i, int k, const MpcWitPlanes &o) {
  const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
  const Fn one = mpc_wit_one(k);
  const Fn left = eval_row(w.rows, rp[0], rp[1], 1, o.aL, o.aR, o.aO, o.v, one, o.chi);
  const Fn right = eval_row(w.rows, rp[1], rp[2], 1, o.aL, o.aR, o.aO, o.v, one, o.chi);
  return mpc_wit_pair(w.op[i], w.arg[i], left, right, o.inputs);
}
// the gate's a_L, a_R into the planes, and d = a_L - x, e = a_R - y of its triple (x, y: this plane's)
BP_HD void mpc_wit_mask_store(const MpcWitPair &g, Words8 *aL, Words8 *aR, const Words8 *x, const Words8 *y, Words8 *d, Words8 *e) {
  wit_store(aL, g.L);
  wit_store(aR, g.R);
  wit_store(d, sub(g.L, load_plain(x)));
  wit_store(e, sub(g.R, load_plain(y)));
}
// slot t of a level of G gates, gate i, plane k of proof p: triples [p][x, y, z][k][t], masked [p][d, e][k][t] (the layouts of
// beaver_term with one product per proof)
BP_HD void mpc_wit_mask_gate(const MpcWitPair &g, uint32_t i, size_t p, int k, size_t G, size_t t, const MpcWitPlanes &o, const Words8 *trip,
                             Words8 *masked) {
  const Words8 *x = trip + (p * 9 + k) * G + t;
  Words8 *d = masked + (p * 6 + k) * G + t;
  mpc_wit_mask_store(g, o.aL + i, o.aR + i, x, x + 3 * G, d, d + 3 * G);
}
BP_HD void mpc_wit_combine_gate(uint32_t i, size_t p, int k, size_t G, size_t t, const MpcWitPlanes &o, const Words8 *opened, const Words8 *trip) {
  wit_store(o.aO + i, beaver_term(opened, trip, p, 1, 0, k, G, t));
}

}  // namespace bpk
