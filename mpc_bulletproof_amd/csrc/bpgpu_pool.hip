// bpgpu_pool.hip -- the bpgpu_pool_* entry points of include/bpgpu.h: queues of independent proofs over several devices from ONE
// process.  A pool is a set of slots: one bpgpu_ctx on one device plus one persistent host thread (pool_workers.hpp) that selects
// the device once and issues every HIP call of its slot.  No arithmetic of its own and no kernel: every slot runs the existing
// single-context entry point on its contiguous share of the queue, and nothing is exchanged on the way but 64 bytes per slot at the
// end of a combined check.  Written on the public entry points, plus bpgpu_internal_verify_stream (bpgpu_internal.h).
#include <hip/hip_runtime.h>
#include <cstring>
#include "pool_host.h"

namespace {

// The in-place operand route of bpgpu_r1cs_verify_stream (the chain's fetch kernel reads page-locked host memory over the bus) is
// taken only when the slice is KNOWN to be mapped for the slot's device: the runtime reports that device as the owner of the first
// and of the last byte, both are device-mapped host memory at one offset from each other, and both lie in one allocation.
// Anything else -- pageable memory, memory page-locked under another device, a query that fails -- takes the staged copies.
bool slice_in_place(int device, const void *p, size_t bytes) {
  if (!bytes) return false;
  const uint8_t *first = (const uint8_t *)p, *last = first + bytes - 1;
  hipPointerAttribute_t a{}, b{};
  if (hipPointerGetAttributes(&a, first) != hipSuccess || hipPointerGetAttributes(&b, last) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (a.type != hipMemoryTypeHost || b.type != hipMemoryTypeHost || a.device != device || b.device != device) return false;
  if (!a.devicePointer || !b.devicePointer) return false;
  if ((const uint8_t *)b.devicePointer - (const uint8_t *)a.devicePointer != (ptrdiff_t)(bytes - 1)) return false;
  hipDeviceptr_t base_a = nullptr, base_b = nullptr;
  size_t size_a = 0, size_b = 0;
  if (hipMemGetAddressRange(&base_a, &size_a, a.devicePointer) != hipSuccess || hipMemGetAddressRange(&base_b, &size_b, b.devicePointer) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return base_a == base_b;
}
// (k < 32) the shape refusals of the verification entry points, from what the pool handles know: padded_n = 2^k must be
// next_pow2(n), the first phase n1 of the n multipliers, and the generators must reach that far
int verify_shape(const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, size_t n1, size_t k) {
  const size_t np = (size_t)1 << k, n = c->n;
  if (n > np || n1 > n || (np > 1 && n <= np / 2 && n != 0)) return BPGPU_E_LEN;
  return np > g->cap ? BPGPU_E_GENS : BPGPU_OK;
}
int circuit_create_any(bpgpu_pool *pool, bool ark, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                       const uint8_t *coeff, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out) {
  if (out) *out = nullptr;
  if (!pool || !out) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    bpgpu_pool_circuit *pc = new bpgpu_pool_circuit();
    pc->pool = pool; pc->n = n_multipliers; pc->m = m_commitments;
    const int rc = make_per_device<bpgpu_circuit>(
        pool, pc->at,
        [&](bpgpu_ctx *ctx, bpgpu_circuit **h) {
          return ark ? bpgpu_circuit_create_ark(ctx, q, row_ptr, kind, idx, coeff, n_multipliers, m_commitments, h)
                     : bpgpu_circuit_create(ctx, q, row_ptr, kind, idx, coeff, n_multipliers, m_commitments, h);
        },
        [](bpgpu_ctx *ctx, bpgpu_circuit *h) { bpgpu_circuit_destroy(ctx, h); }, ark ? "bpgpu_pool_circuit_create_ark" : "bpgpu_pool_circuit_create");
    if (rc) { delete pc; return rc; }
    *out = pc;
    return BPGPU_OK;
  });
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int bpgpu_pool_shares(size_t nb, size_t nslots, size_t granule, size_t *lo) {
  if (!nslots || !granule || !lo) return BPGPU_E_ARG;
  const size_t granules = nb / granule + (nb % granule ? 1 : 0), base = granules / nslots, extra = granules % nslots;
  size_t taken = 0;      // granules of the slots before s
  lo[0] = 0;
  for (size_t s = 0; s < nslots; s++) {
    taken += base + (s < extra ? 1 : 0);
    lo[s + 1] = taken >= granules ? nb : taken * granule;     // (the last granule may be short; taken < granules: no overflow below nb)
  }
  return BPGPU_OK;
}

int bpgpu_pool_create(const int *devices, size_t nslots, bpgpu_pool **out) {
  if (out) *out = nullptr;
  if (!out || !devices || !nslots || nslots > BPGPU_POOL_MAX_SLOTS) return BPGPU_E_ARG;
  const int count = bpgpu_device_count();
  if (count <= 0) return BPGPU_E_DEVICE;
  for (size_t s = 0; s < nslots; s++)
    if (devices[s] < 0 || devices[s] >= count) return BPGPU_E_DEVICE;
  return noexcept_abi([&]() -> int {
    bpgpu_pool *pool = new bpgpu_pool();
    pool->device.assign(devices, devices + nslots);
    pool->ctx.assign(nslots, nullptr);
    pool->owner.assign(nslots, 0);
    for (size_t s = 0; s < nslots; s++) {
      size_t o = 0;
      while (devices[o] != devices[s]) o++;
      pool->owner[s] = o;
    }
    if (!pool->workers.start(nslots, [pool](size_t s) { (void)hipSetDevice(pool->device[s]); })) { delete pool; return BPGPU_E_OOM; }
    std::vector<Job> jobs(nslots);
    for (size_t s = 0; s < nslots; s++) jobs[s] = [pool, s]() -> int { return bpgpu_create(pool->device[s], &pool->ctx[s]); };
    std::vector<int> codes;
    const long bad = pool->workers.run(jobs, codes);
    if (bad >= 0) {
      const int rc = codes[(size_t)bad];
      bpgpu_pool_destroy(pool);
      return rc;
    }
    *out = pool;
    return BPGPU_OK;
  });
}
void bpgpu_pool_destroy(bpgpu_pool *pool) {
  if (!pool) return;
  try {
    std::vector<Job> jobs(pool->ctx.size());
    for (size_t s = 0; s < pool->ctx.size(); s++)
      if (pool->ctx[s]) jobs[s] = [pool, s]() -> int { bpgpu_destroy(pool->ctx[s]); pool->ctx[s] = nullptr; return 0; };
    std::vector<int> codes;
    pool->workers.run(jobs, codes);
  } catch (const std::bad_alloc &) {
    for (bpgpu_ctx *&c : pool->ctx) { bpgpu_destroy(c); c = nullptr; }    // (bpgpu_destroy selects the device itself)
  }
  pool->workers.stop();
  delete pool;
}
size_t bpgpu_pool_slots(const bpgpu_pool *pool) { return pool ? pool->ctx.size() : 0; }
int bpgpu_pool_device(const bpgpu_pool *pool, size_t slot) { return pool && slot < pool->device.size() ? pool->device[slot] : BPGPU_E_ARG; }
bpgpu_ctx *bpgpu_pool_ctx(bpgpu_pool *pool, size_t slot) { return pool && slot < pool->ctx.size() ? pool->ctx[slot] : nullptr; }
const char *bpgpu_pool_last_error(bpgpu_pool *pool) { return pool ? pool->err.c_str() : ""; }

int bpgpu_pool_set_option(bpgpu_pool *pool, int option, int64_t value) {
  if (!pool) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const size_t ns = pool->ctx.size();
    std::vector<int64_t> old(ns, 0);
    for (size_t s = 0; s < ns; s++) {
      int rc = bpgpu_get_option(pool->ctx[s], option, &old[s]);
      if (!rc) rc = bpgpu_set_option(pool->ctx[s], option, value);
      if (rc) {                                            // all or nothing: the slots already set get their values back
        for (size_t t = 0; t < s; t++) (void)bpgpu_set_option(pool->ctx[t], option, old[t]);
        return refuse(pool, rc, "bpgpu_pool_set_option");
      }
    }
    return BPGPU_OK;
  });
}

int bpgpu_pool_gens_create(bpgpu_pool *pool, const uint8_t *G, const uint8_t *H, size_t gens_capacity, const uint8_t B[64],
                           const uint8_t B_blinding[64], int window_bits, bpgpu_pool_gens **out) {
  if (out) *out = nullptr;
  if (!pool || !out) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    bpgpu_pool_gens *pg = new bpgpu_pool_gens();
    pg->pool = pool; pg->cap = gens_capacity;
    const int rc = make_per_device<bpgpu_gens>(
        pool, pg->at, [&](bpgpu_ctx *ctx, bpgpu_gens **h) { return bpgpu_gens_create(ctx, G, H, gens_capacity, B, B_blinding, window_bits, h); },
        [](bpgpu_ctx *ctx, bpgpu_gens *h) { bpgpu_gens_destroy(ctx, h); }, "bpgpu_pool_gens_create");
    if (rc) { delete pg; return rc; }
    *out = pg;
    return BPGPU_OK;
  });
}
void bpgpu_pool_gens_destroy(bpgpu_pool *pool, bpgpu_pool_gens *g) {
  if (!pool || !g || g->pool != pool) return;
  try {
    std::lock_guard<std::mutex> lk(pool->mu);
    drop_per_device<bpgpu_gens>(pool, g->at, [](bpgpu_ctx *ctx, bpgpu_gens *h) { bpgpu_gens_destroy(ctx, h); });
  } catch (const std::bad_alloc &) {
  }
  delete g;
}
const bpgpu_gens *bpgpu_pool_gens_get(const bpgpu_pool_gens *g, size_t slot) { return g && slot < g->at.size() ? g->at[slot] : nullptr; }

int bpgpu_pool_circuit_create(bpgpu_pool *pool, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                              const uint8_t *coeff, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out) {
  return circuit_create_any(pool, false, q, row_ptr, kind, idx, coeff, n_multipliers, m_commitments, out);
}
int bpgpu_pool_circuit_create_ark(bpgpu_pool *pool, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                                  const uint8_t *coeff_ark, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out) {
  return circuit_create_any(pool, true, q, row_ptr, kind, idx, coeff_ark, n_multipliers, m_commitments, out);
}
void bpgpu_pool_circuit_destroy(bpgpu_pool *pool, bpgpu_pool_circuit *c) {
  if (!pool || !c || c->pool != pool) return;
  try {
    std::lock_guard<std::mutex> lk(pool->mu);
    drop_per_device<bpgpu_circuit>(pool, c->at, [](bpgpu_ctx *ctx, bpgpu_circuit *h) { bpgpu_circuit_destroy(ctx, h); });
  } catch (const std::bad_alloc &) {
  }
  delete c;
}
const bpgpu_circuit *bpgpu_pool_circuit_get(const bpgpu_pool_circuit *c, size_t slot) { return c && slot < c->at.size() ? c->at[slot] : nullptr; }

int bpgpu_pool_r1cs_verify_stream(bpgpu_pool *pool, const bpgpu_pool_gens *pg, const bpgpu_pool_circuit *pc, size_t nb, size_t n1, size_t k,
                                  const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, int32_t *ok, size_t *slot_proofs) {
  if (!numeric_ok(pool, pg, pc) || (nb && (!points || !scalars || !challenges || !ok))) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const char *what = "bpgpu_pool_r1cs_verify_stream";
    if (!nb) return BPGPU_OK;
    if (k >= 32) return refuse(pool, BPGPU_E_LEN, what);
    if (const int rc = verify_shape(pg, pc, n1, k)) return refuse(pool, rc, what);
    const size_t ns = pool->ctx.size(), bp = (11 + pc->m + 2 * k) * 64, bs = 5 * 32, bc = (6 + k) * 32;
    std::vector<size_t> lo;
    if (const int rc = shares_of(pool, nb, BPGPU_OPT_STREAM_BATCH, lo)) return refuse(pool, rc, what);
    std::vector<Job> jobs(ns);
    for (size_t s = 0; s < ns; s++) {
      const size_t a = lo[s], cnt = lo[s + 1] - lo[s];
      if (slot_proofs) slot_proofs[s] = cnt;
      if (!cnt) continue;
      jobs[s] = [=]() -> int {
        const uint8_t *P = points + a * bp, *S = scalars + a * bs, *Cc = challenges + a * bc;
        const int dev = pool->device[s];
        const int in_place = slice_in_place(dev, P, cnt * bp) && slice_in_place(dev, S, cnt * bs) && slice_in_place(dev, Cc, cnt * bc);
        return bpgpu_internal_verify_stream(pool->ctx[s], pg->at[s], pc->at[s], cnt, n1, k, P, S, Cc, ok + a, in_place);
      };
    }
    return run_slots(pool, jobs, what);
  });
}

int bpgpu_pool_r1cs_verify_screened(bpgpu_pool *pool, const bpgpu_pool_gens *pg, const bpgpu_pool_circuit *pc, size_t nb, size_t n1, size_t k,
                                    const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, int32_t *ok,
                                    size_t *fallback_batches) {
  if (!numeric_ok(pool, pg, pc) || (nb && (!points || !scalars || !challenges || !rho || !ok))) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const char *what = "bpgpu_pool_r1cs_verify_screened";
    if (!nb) return BPGPU_OK;
    if (k >= 32) return refuse(pool, BPGPU_E_LEN, what);
    if (const int rc = verify_shape(pg, pc, n1, k)) return refuse(pool, rc, what);
    const size_t ns = pool->ctx.size(), bp = (11 + pc->m + 2 * k) * 64, bs = 5 * 32, bc = (6 + k) * 32;
    std::vector<size_t> lo, fell(ns, 0);
    if (const int rc = shares_of(pool, nb, BPGPU_OPT_SCREEN_BATCH, lo)) return refuse(pool, rc, what);
    std::vector<Job> jobs(ns);
    for (size_t s = 0; s < ns; s++) {
      const size_t a = lo[s], cnt = lo[s + 1] - lo[s];
      if (!cnt) continue;
      size_t *nf = &fell[s];
      jobs[s] = [=]() -> int {
        return bpgpu_r1cs_verify_screened(pool->ctx[s], pg->at[s], pc->at[s], cnt, n1, k, points + a * bp, scalars + a * bs, challenges + a * bc,
                                          rho + a * 32, ok + a, nf);
      };
    }
    const int rc = run_slots(pool, jobs, what);
    if (fallback_batches) {
      *fallback_batches = 0;
      for (size_t f : fell) *fallback_batches += f;
    }
    return rc;
  });
}

int bpgpu_pool_r1cs_verify_combined(bpgpu_pool *pool, const bpgpu_pool_gens *pg, const bpgpu_pool_circuit *pc, size_t nb, size_t n1, size_t k,
                                    const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho,
                                    uint8_t out_xy[64]) {
  if (!numeric_ok(pool, pg, pc) || (nb && (!points || !scalars || !challenges || !rho)) || !out_xy) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const char *what = "bpgpu_pool_r1cs_verify_combined";
    if (!nb) return BPGPU_OK;
    if (k >= 32) return refuse(pool, BPGPU_E_LEN, what);
    if (const int rc = verify_shape(pg, pc, n1, k)) return refuse(pool, rc, what);
    const size_t ns = pool->ctx.size(), bp = (11 + pc->m + 2 * k) * 64, bs = 5 * 32, bc = (6 + k) * 32;
    std::vector<size_t> lo;
    if (const int rc = shares_of(pool, nb, BPGPU_OPT_SCREEN_BATCH, lo)) return refuse(pool, rc, what);
    std::vector<uint8_t> partial(ns * 64, 0);       // slot s's point at 64 s, then packed to the front for the sum
    std::vector<Job> jobs(ns);
    for (size_t s = 0; s < ns; s++) {
      const size_t a = lo[s], cnt = lo[s + 1] - lo[s];
      if (!cnt) continue;
      uint8_t *mine = partial.data() + 64 * s;
      jobs[s] = [=]() -> int {
        return bpgpu_r1cs_verify_combined(pool->ctx[s], pg->at[s], pc->at[s], cnt, n1, k, points + a * bp, scalars + a * bs, challenges + a * bc,
                                          rho + a * 32, mine);
      };
    }
    if (const int rc = run_slots(pool, jobs, what)) return rc;
    // the reduction: 64 bytes per non-empty slot, added on slot 0 (between processes this is the all-gather of the partials)
    size_t np = 0;
    for (size_t s = 0; s < ns; s++)
      if (lo[s + 1] > lo[s]) { if (np != s) memcpy(partial.data() + 64 * np, partial.data() + 64 * s, 64); np++; }
    std::vector<Job> sum(ns);
    sum[0] = [&]() -> int { return bpgpu_points_sum(pool->ctx[0], partial.data(), np, out_xy); };
    return run_slots(pool, sum, what);
  });
}

int bpgpu_pool_r1cs_prove_fs(bpgpu_pool *pool, const bpgpu_pool_gens *pg, const bpgpu_pool_circuit *pc, size_t nb, const uint8_t *states_in,
                             const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                             const uint8_t *vector_keys, const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points,
                             uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out) {
  if (!numeric_ok(pool, pg, pc)) return BPGPU_E_ARG;
  return noexcept_abi([&]() -> int {
    std::lock_guard<std::mutex> lk(pool->mu);
    const char *what = "bpgpu_pool_r1cs_prove_fs";
    if (!nb) return BPGPU_OK;
    // the refusals of bpgpu_r1cs_prove_fs that depend on shapes and arguments alone, in its order
    const size_t n = pc->n, m = pc->m;
    if (!n) return refuse(pool, BPGPU_E_LEN, what);
    size_t padded_n = 1, k = 0;
    while (padded_n < n) { padded_n <<= 1; k++; }
    if (padded_n > pg->cap) return refuse(pool, BPGPU_E_GENS, what);
    if (!states_in || !a_L || !a_R || !a_O || !blindings || !proof_points || !proof_scalars || (m && !v_blinding)) return refuse(pool, BPGPU_E_ARG, what);
    if ((!s_L) != (!s_R) || (s_L != nullptr) == (vector_keys != nullptr)) return refuse(pool, BPGPU_E_ARG, what);
    const size_t ns = pool->ctx.size(), bw = n * 32, bpts = (11 + 2 * k) * 64, bwire = 1 + 11 * 32 + (2 * k + 2) * 32, bch = (5 + k) * 32;
    std::vector<size_t> lo;
    if (const int rc = shares_of(pool, nb, 0, lo)) return refuse(pool, rc, what);
    std::vector<Job> jobs(ns);
    for (size_t s = 0; s < ns; s++) {
      const size_t a = lo[s], cnt = lo[s + 1] - lo[s];
      if (!cnt) continue;
      jobs[s] = [=]() -> int {
        return bpgpu_r1cs_prove_fs(pool->ctx[s], pg->at[s], pc->at[s], cnt, states_in + a * 32, a_L + a * bw, a_R + a * bw, a_O + a * bw,
                                   at(s_L, a * bw), at(s_R, a * bw), at(vector_keys, a * 32), at(v_blinding, a * m * 32), blindings + a * 8 * 32,
                                   proof_points + a * bpts, proof_scalars + a * 5 * 32, at(wire, a * bwire), at(challenges_out, a * bch),
                                   at(states_out, a * 32));
      };
    }
    return run_slots(pool, jobs, what);
  });
}

#pragma GCC visibility pop
}
