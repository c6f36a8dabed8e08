// witness_dev.cuh -- one gate of a bpgpu_witness program (Prover::multiply, prover.rs:99-125; allocate_multiplier, :148-165; the range
// gadget's bit assignment, tests/r1cs.rs:629-632): what every lane of k_witness.hip runs, and what tests/csrc/witness_host_test.cpp
// compiles for the CPU.  The row sums are eval_row's (fn_dev.cuh): lazy, reduced here before the gate's product.
#pragma once
#include "fn_dev.cuh"

namespace bpk {

constexpr uint32_t WIT_OP_MUL = 0, WIT_OP_INPUT = 1, WIT_OP_BIT = 2;   // BPGPU_GATE_* of include/bpgpu.h
constexpr uint32_t WIT_BIT_MAX = 252;                                  // a BIT gate reads a bit below this one

struct WitGate { Fn L, R, O; };

BP_HD void wit_store(Words8 *p, const Fn &x) {   // Montgomery -> plain canonical words
  uint32_t w[8];
  pack(w, from_mont(x));
#pragma unroll
  for (int j = 0; j < 8; j++) p->w[j] = w[j];
}
// The gate's three values from the lazy sums of its two rows.  Both operands of the product are reduced first: mul documents
// |v| < 2^256 for two general operands, and a lazy sum of 16 products is far above that.  `inputs`: the prover's pairs (plain words);
// arg: the pair of an INPUT gate, the bit (< WIT_BIT_MAX) of a BIT gate.
BP_HD WitGate wit_gate_values(uint32_t op, uint32_t arg, const Fn &left, const Fn &right, const Words8 *inputs) {
  WitGate g;
  if (op == WIT_OP_INPUT) {
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
// gate i of one prover, both rows by this lane; aL, aR, aO, v, inputs, chi: the prover's own (plain canonical words)
BP_HD void wit_gate_lane(const WitDev &w, uint32_t i, Words8 *aL, Words8 *aR, Words8 *aO, const Words8 *v, const Words8 *inputs,
                         const Words8 *chi) {
  const uint32_t *rp = w.rows.row_ptr + 2 * (size_t)i;
  const Fn one = fe_one<FN>();
  const Fn left = eval_row(w.rows, rp[0], rp[1], 1, aL, aR, aO, v, one, chi);
  const Fn right = eval_row(w.rows, rp[1], rp[2], 1, aL, aR, aO, v, one, chi);
  const WitGate g = wit_gate_values(w.op[i], w.arg[i], left, right, inputs);
  wit_store(aL + i, g.L);
  wit_store(aR + i, g.R);
  wit_store(aO + i, g.O);
}

}  // namespace bpk
