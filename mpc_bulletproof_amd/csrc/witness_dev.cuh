// witness_dev.cuh -- one gate of a bpgpu_witness program (Prover::multiply, prover.rs:99-125; allocate_multiplier, :148-165; the range
// gadget's bit assignment, tests/r1cs.rs:629-632): what every lane of k_witness.hip runs, and what tests/csrc/witness_host_test.cpp
// compiles for the CPU.  The row sums are eval_row's (fn_dev.cuh): lazy, reduced here before the gate's product.
#pragma once
#include "fn_dev.cuh"
#include "int_div.cuh"

namespace bpk {

constexpr uint32_t WIT_OP_MUL = 0, WIT_OP_INPUT = 1, WIT_OP_BIT = 2, WIT_OP_INV = 4;   // BPGPU_GATE_* of include/bpgpu.h (3 is no op)
constexpr uint32_t WIT_OP_DIVREM = 6;                                  // (and neither is 5)
constexpr uint32_t WIT_BIT_MAX = 252;                                  // a BIT gate reads a bit below this one

struct WitGate { Fn L, R, O; };

BP_HD void wit_store(Words8 *p, const Fn &x) {   // Montgomery -> plain canonical words
  uint32_t w[8];
  pack(w, from_mont(x));
#pragma unroll
  for (int j = 0; j < 8; j++) p->w[j] = w[j];
}
// the same, and whether any of the words written is set: the zero test of an INV gate, on the canonical integer
BP_HD bool wit_store_nz(Words8 *p, const Fn &x) {
  uint32_t w[8], any = 0;
  pack(w, from_mont(x));
#pragma unroll
  for (int j = 0; j < 8; j++) { p->w[j] = w[j]; any |= w[j]; }
  return any != 0;
}
// A DIVREM gate's quotient and remainder words from the lazy sums of its two rows: x and y are the CANONICAL integers of the rows
// (a value left lazily at v + n, or negative, has another quotient), brought there the way the BIT gate brings its integer.
BP_HD void wit_divrem_words(uint32_t (&q)[8], uint32_t (&r)[8], const Fn &left, const Fn &right) {
  uint32_t x[8], y[8];
  pack(x, from_mont(fn_reduce(left)));
  pack(y, from_mont(fn_reduce(right)));
  int_divrem(q, r, x, y);
}
// The gate's three values from the lazy sums of its two rows.  Both operands of the product are reduced first: mul documents
// |v| < 2^256 for two general operands, and a lazy sum of 16 products is far above that.  `inputs`: the prover's pairs (plain words);
// arg: the pair of an INPUT gate, the bit (< WIT_BIT_MAX) of a BIT gate.  INV: whether the caller's program may hold an INV gate (a
// kernel of a phase without one carries no inversion: k_witness.hip); DIV: the same for a DIVREM gate and the integer division.
template <bool INV, bool DIV = false>
BP_HD WitGate wit_gate_values_of(uint32_t op, uint32_t arg, const Fn &left, const Fn &right, const Words8 *inputs) {
  WitGate g;
  if (DIV && op == WIT_OP_DIVREM) {
    // q and r are canonical integers below n (q <= x, r <= x): unpack gives tight limbs, to_mont the Montgomery form
    uint32_t q[8], r[8];
    wit_divrem_words(q, r, left, right);
    g.L = to_mont(unpack<FN>(q));
    g.R = to_mont(unpack<FN>(r));
  } else if (INV && op == WIT_OP_INV) {
    // inverse-or-zero: inv maps 0 to 0, so a zero a_L gives a_R = a_O = 0 with no test (0 in any lazy form is 0 mod n).  inv's
    // result has lazy signed limbs of magnitude below 2^29 and |value| < 2 n < 2^256: an operand mul takes as it stands (fe29.cuh:
    // the bounds are on magnitudes), so it feeds the gate's product, and wit_store's from_mont, without a reduction.
    g.L = fn_reduce(left);
    g.R = inv(g.L);
  } else if (op == WIT_OP_INPUT) {
    g.L = load_plain(inputs + 2 * (size_t)arg);
    g.R = load_plain(inputs + 2 * (size_t)arg + 1);
  } else if (op == WIT_OP_BIT) {
    uint32_t w[8], word = 0;
    pack(w, from_mont(fn_reduce(left)));          // the canonical integer of eval(left)
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) word = (j == (arg >> 5)) ? w[j] : word;   // (no dynamic index into registers)
    const bool b = (word >> (arg & 31)) & 1u;
    g.L = b ? fe_zero<FN>() : fe_one<FN>();
    g.R = b ? fe_one<FN>() : fe_zero<FN>();
  } else {
    g.L = fn_reduce(left);
    g.R = fn_reduce(right);
  }
  g.O = mul(g.L, g.R);
  return g;
}
BP_HD WitGate wit_gate_values(uint32_t op, uint32_t arg, const Fn &left, const Fn &right, const Words8 *inputs) {
  return wit_gate_values_of<true, true>(op, arg, left, right, inputs);
}
// ... and stored: a_L and a_R of a DIVREM gate as the plain words the division produced, a_O from them; every other gate as
// wit_gate_values_of has it
template <bool INV, bool DIV = false>
BP_HD void wit_gate_store_of(uint32_t op, uint32_t arg, const Fn &left, const Fn &right, const Words8 *inputs, Words8 *pL, Words8 *pR,
                             Words8 *pO) {
  if (DIV && op == WIT_OP_DIVREM) {
    uint32_t q[8], r[8];
    wit_divrem_words(q, r, left, right);
#pragma unroll
    for (int j = 0; j < 8; j++) { pL->w[j] = q[j]; pR->w[j] = r[j]; }
    wit_store(pO, mul(to_mont(unpack<FN>(q)), to_mont(unpack<FN>(r))));
    return;
  }
  const WitGate g = wit_gate_values_of<INV, false>(op, arg, left, right, inputs);
  wit_store(pL, g.L);
  wit_store(pR, g.R);
  wit_store(pO, g.O);
}
// gate i of one prover, both rows by this lane; aL, aR, aO, v, inputs, chi: the prover's own (plain canonical words)
template <bool INV, bool DIV = false>
BP_HD void wit_gate_lane_of(const WitDev &w, uint32_t i, Words8 *aL, Words8 *aR, Words8 *aO, const Words8 *v, const Words8 *inputs,
                            const Words8 *chi) {
  const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
  const Fn one = fe_one<FN>();
  const Fn left = eval_row(w.rows, rp[0], rp[1], 1, aL, aR, aO, v, one, chi);
  const Fn right = eval_row(w.rows, rp[1], rp[2], 1, aL, aR, aO, v, one, chi);
  if (DIV) {                 // (a kernel without the op keeps the statements it always had)
    wit_gate_store_of<INV, DIV>(w.op[i], w.arg[i], left, right, inputs, aL + i, aR + i, aO + i);
    return;
  }
  const WitGate g = wit_gate_values_of<INV>(w.op[i], w.arg[i], left, right, inputs);
  wit_store(aL + i, g.L);
  wit_store(aR + i, g.R);
  wit_store(aO + i, g.O);
}
BP_HD void wit_gate_lane(const WitDev &w, uint32_t i, Words8 *aL, Words8 *aR, Words8 *aO, const Words8 *v, const Words8 *inputs,
                         const Words8 *chi) {
  wit_gate_lane_of<true, true>(w, i, aL, aR, aO, v, inputs, chi);
}

// ---- a level's INV gates with ONE inversion per thread (Montgomery's trick) -----------------------------------------------------------
// A thread owns the gates order[first], order[first + step], .. below hi (k_witness.hip: first = the level's first INV gate + the
// thread, step = 256).  Forward: a_L of each is stored (final), the running product of the NON-ZERO a_L so far is parked in the
// gate's a_R slot -- as the canonical Montgomery words of the product BEFORE this gate, which only this thread reads back: the gates
// that read the slot sit on later levels -- and a non-zero a_L is multiplied in (a zero one counts as the factor 1).  The caller
// inverts what comes back, once.  Backward, last gate first: a_R = running^-1 * parked, running^-1 *= a_L, a_O = 1; a zero gate
// gets a_R = a_O = 0 and leaves running^-1 alone.  The zero test is wit_store_nz's, on the words stored; backward reads it off a_L.
// A thread without a gate, or with zero gates only, has the product 1, whose inverse is 1: no special case.
// Limb bound: every factor is fn_reduce's output (a mul output: tight limbs, within one modulus of zero) and so is every product;
// inv's result is an operand mul takes as it stands (wit_gate_values_of) and after the first backward step a mul output again;
// the parked words unpack to a tight value below n.  All inside |v| < 2^256: products feed products for any run length.
BP_HD Fn wit_inv_forward(const WitDev &w, const uint32_t *order, uint32_t first, uint32_t hi, uint32_t step, Words8 *aL, Words8 *aR,
                         Words8 *aO, const Words8 *v, const Words8 *chi) {
  Fn run = fe_one<FN>();
  const Fn one = fe_one<FN>();
  for (uint32_t t = first; t < hi; t += step) {
    const uint32_t i = order[t];
    const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
    const Fn x = fn_reduce(eval_row(w.rows, rp[0], rp[1], 1, aL, aR, aO, v, one, chi));
    uint32_t pw[8];
    pack(pw, canon(run));
#pragma unroll
    for (int j = 0; j < 8; j++) aR[i].w[j] = pw[j];
    const bool nz = wit_store_nz(aL + i, x);
    const Fn both = mul(run, x);
#pragma unroll
    for (int j = 0; j < NL; j++) run.v[j] = nz ? both.v[j] : run.v[j];
  }
  return run;
}
// run_inv: the inverse of what wit_inv_forward returned for the same gates
BP_HD void wit_inv_backward(const uint32_t *order, uint32_t first, uint32_t hi, uint32_t step, Fn run_inv, Words8 *aL, Words8 *aR,
                            Words8 *aO) {
  if (first >= hi) return;
  const Fn one = fe_one<FN>(), zero = fe_zero<FN>();
  for (uint32_t k = (hi - first + step - 1) / step; k-- > 0;) {
    const uint32_t i = order[first + k * step];
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) any |= aL[i].w[j];
    const bool nz = any != 0;
    const Fn r = mul(run_inv, load_words(aR + i)), next = mul(run_inv, load_plain(aL + i));
    wit_store(aR + i, nz ? r : zero);
    wit_store(aO + i, nz ? one : zero);
#pragma unroll
    for (int j = 0; j < NL; j++) run_inv.v[j] = nz ? next.v[j] : run_inv.v[j];
  }
}

}  // namespace bpk
