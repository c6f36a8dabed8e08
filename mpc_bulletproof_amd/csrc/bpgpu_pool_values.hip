// bpgpu_pool_values.hip -- the pool forms of the prover's front end (include/bpgpu.h): parametric circuits and bpgpu_witness gate
// programs per distinct device, and bpgpu_pool_r1cs_prove_values, which deals bpgpu_r1cs_prove_values over the slots.  Host code only,
// written on the public entry points plus the call's own refusals (bpgpu_internal.h); the pool itself is bpgpu_pool.hip.
#include <hip/hip_runtime.h>
#include <cstring>

#include "pool_host.h"

extern "C" {
#pragma GCC visibility push(default)

int bpgpu_pool_circuit_create_param(bpgpu_pool *pool, size_t q, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                                    const uint8_t *coeff, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out) {
  if (out) *out = nullptr;
  if (!pool || !out) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    bpgpu_pool_circuit *pc = new bpgpu_pool_circuit();
    pc->pool = pool; pc->n = n_multipliers; pc->m = m_commitments; pc->nchi = nchi;
    const int rc = make_per_device<bpgpu_circuit>(
        pool, pc->at,
        [&](bpgpu_ctx *ctx, bpgpu_circuit **h) { return bpgpu_circuit_create_param(ctx, q, nchi, row_ptr, kind, idx, coeff, n_multipliers, m_commitments, h); },
        [](bpgpu_ctx *ctx, bpgpu_circuit *h) { bpgpu_circuit_destroy(ctx, h); }, "bpgpu_pool_circuit_create_param");
    if (rc) { delete pc; return rc; }
    *out = pc;
    return BPGPU_OK;
  });
}
int bpgpu_pool_circuit_set_gadget_labels(bpgpu_pool *pool, bpgpu_pool_circuit *pc, const uint8_t *labels) {
  if (!pool || !pc || pc->pool != pool || !labels) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    for (size_t s = 0; s < pc->at.size(); s++) {    // (slots of one device share their owner's handle; no pool call runs meanwhile)
      if (pool->owner[s] != s) continue;
      if (const int rc = bpgpu_circuit_set_gadget_labels(pool->ctx[s], pc->at[s], labels)) return refuse(pool, rc, "bpgpu_pool_circuit_set_gadget_labels");
    }
    return BPGPU_OK;
  });
}
int bpgpu_pool_witness_create(bpgpu_pool *pool, size_t n, size_t n1, size_t m, size_t nchi, const uint8_t *op, const uint32_t *arg,
                              const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx, const uint8_t *coeff, bpgpu_pool_witness **out) {
  if (out) *out = nullptr;
  if (!pool || !out) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    bpgpu_pool_witness *pw = new bpgpu_pool_witness();
    pw->pool = pool;
    const int rc = make_per_device<bpgpu_witness>(
        pool, pw->at, [&](bpgpu_ctx *ctx, bpgpu_witness **h) { return bpgpu_witness_create(ctx, n, n1, m, nchi, op, arg, row_ptr, kind, idx, coeff, h); },
        [](bpgpu_ctx *ctx, bpgpu_witness *h) { bpgpu_witness_destroy(ctx, h); }, "bpgpu_pool_witness_create");
    if (rc) { delete pw; return rc; }
    pw->ninp = bpgpu_internal_witness_inputs(pw->at[0]);
    *out = pw;
    return BPGPU_OK;
  });
}
void bpgpu_pool_witness_destroy(bpgpu_pool *pool, bpgpu_pool_witness *w) {
  if (!pool || !w || w->pool != pool) return;
  try {
    std::lock_guard<std::mutex> lk(pool->mu);
    drop_per_device<bpgpu_witness>(pool, w->at, [](bpgpu_ctx *ctx, bpgpu_witness *h) { bpgpu_witness_destroy(ctx, h); });
  } catch (const std::bad_alloc &) {
  }
  delete w;
}
const bpgpu_witness *bpgpu_pool_witness_get(const bpgpu_pool_witness *w, size_t slot) { return w && slot < w->at.size() ? w->at[slot] : nullptr; }

int bpgpu_pool_r1cs_prove_values(bpgpu_pool *pool, const bpgpu_pool_gens *pg, const bpgpu_pool_circuit *pc, const bpgpu_pool_witness *pw, size_t nb,
                                 const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *v, const uint8_t *v_blinding,
                                 const uint8_t *inputs, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys,
                                 const uint8_t *blindings, uint8_t *V, uint8_t *V_compressed, int32_t *ok, int64_t *first_bad_row,
                                 int64_t *first_bad_gate, uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out,
                                 uint8_t *states_out, uint8_t *gadget_challenges_out, uint8_t *a_L_out, uint8_t *a_R_out, uint8_t *a_O_out) {
  if (!handles_ok(pool, pg, pc) || !pw || pw->pool != pool) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const char *what = "bpgpu_pool_r1cs_prove_values";
    if (!nb) return BPGPU_OK;
    const size_t ns = pool->ctx.size();
    std::vector<size_t> lo;
    if (const int rc = shares_of(pool, nb, 0, lo)) return refuse(pool, rc, what);
    // the refusals of bpgpu_r1cs_prove_values, per non-empty slot on its own handles and context: nothing of them needs a device
    const bpgpu_internal_pv whole{init_states, gadget_label, v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, V, V_compressed, ok,
                                  first_bad_row, first_bad_gate, proof_points, proof_scalars, wire, challenges_out, states_out,
                                  gadget_challenges_out, a_L_out, a_R_out, a_O_out};
    for (size_t s = 0; s < ns; s++)
      if (lo[s + 1] > lo[s])
        if (const int rc = bpgpu_internal_prove_values_check(pool->ctx[s], pg->at[s], pc->at[s], pw->at[s], lo[s + 1] - lo[s], whole))
          return refuse(pool, rc, what);
    const bool two = pc->nchi != 0;
    size_t k = 0;
    while (((size_t)1 << k) < pc->n) k++;
    const size_t m = pc->m, bw = pc->n * 32, bin = 2 * pw->ninp * 32, bkey = two ? 64 : 32, bbl = (two ? 11 : 8) * 32, bpts = (11 + 2 * k) * 64,
                 bwire = 1 + (two ? 14 : 11) * 32 + (2 * k + 2) * 32, bch = (5 + k) * 32;
    std::vector<Job> jobs(ns);
    for (size_t s = 0; s < ns; s++) {
      const size_t a = lo[s], cnt = lo[s + 1] - lo[s];
      if (!cnt) continue;
      jobs[s] = [=]() -> int {
        return bpgpu_r1cs_prove_values(pool->ctx[s], pg->at[s], pc->at[s], pw->at[s], cnt, init_states + a * 32, gadget_label, at(v, a * m * 32),
                                       at(v_blinding, a * m * 32), at(inputs, a * bin), at(s_L, a * bw), at(s_R, a * bw), at(vector_keys, a * bkey),
                                       blindings + a * bbl, at(V, a * m * 64), at(V_compressed, a * m * 32), ok + a,
                                       first_bad_row ? first_bad_row + a : nullptr, first_bad_gate ? first_bad_gate + a : nullptr,
                                       proof_points + a * bpts, proof_scalars + a * 5 * 32, at(wire, a * bwire), at(challenges_out, a * bch),
                                       at(states_out, a * 32), at(gadget_challenges_out, a * pc->nchi * 32), at(a_L_out, a * bw), at(a_R_out, a * bw),
                                       at(a_O_out, a * bw));
      };
    }
    return run_slots(pool, jobs, what);
  });
}

#pragma GCC visibility pop
}
