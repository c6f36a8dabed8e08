// pool_host.h -- what the two host files of the pools share (bpgpu_pool.hip: pools, their generators and numeric circuits, the
// verification calls and bpgpu_pool_r1cs_prove_fs; bpgpu_pool_values.hip: parametric circuits, gate programs and
// bpgpu_pool_r1cs_prove_values): the handles and the scaffolding of a pool call.  Not exported.
#ifndef BPGPU_POOL_HOST_H
#define BPGPU_POOL_HOST_H
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "bpgpu_internal.h"
#include "pool_workers.hpp"

struct bpgpu_pool {
  std::mutex mu;                     // one pool call at a time
  std::vector<int> device;           // per slot
  std::vector<bpgpu_ctx *> ctx;      // per slot
  std::vector<size_t> owner;         // per slot: the lowest slot of the same device, which creates and destroys that device's handles
  bppool::Workers workers{BPGPU_E_OOM};   // (a job that throws has run out of host memory: nothing else in them throws)
  std::string err;
};
// one handle per distinct device, shared by that device's slots
struct bpgpu_pool_gens {
  const bpgpu_pool *pool = nullptr;
  std::vector<bpgpu_gens *> at;      // per slot (at[s] == at[owner[s]])
  size_t cap = 0;
};
struct bpgpu_pool_circuit {
  const bpgpu_pool *pool = nullptr;
  std::vector<bpgpu_circuit *> at;
  size_t n = 0, m = 0;               // multipliers, commitments: the strides of a proof's operands
  size_t nchi = 0;                   // gadget challenges: > 0 for a handle of bpgpu_pool_circuit_create_param, which only
                                     // bpgpu_pool_r1cs_prove_values takes
};
struct bpgpu_pool_witness {
  const bpgpu_pool *pool = nullptr;
  std::vector<bpgpu_witness *> at;
  size_t ninp = 0;                   // INPUT pairs per prover: the stride of `inputs` (the others are the circuit's n and m)
};

namespace {

using Job = bppool::Workers::Job;

// one round on the workers; the error of the lowest failing slot, with its slot, device and context text in pool->err
int run_slots(bpgpu_pool *pool, const std::vector<Job> &jobs, const char *what) {
  std::vector<int> codes;
  const long bad = pool->workers.run(jobs, codes);
  if (bad < 0) return BPGPU_OK;
  const size_t s = (size_t)bad;
  pool->err = std::string(what) + ": slot " + std::to_string(s) + " (device " + std::to_string(pool->device[s]) + "): " +
              bpgpu_strerror(codes[s]) + " | " + bpgpu_last_error(pool->ctx[s]);
  return codes[s];
}
int refuse(bpgpu_pool *pool, int code, const char *what) {
  pool->err = std::string(what) + ": " + bpgpu_strerror(code) + " (refused before any slot was woken)";
  return code;
}
bool handles_ok(const bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c) {
  return pool && g && c && g->pool == pool && c->pool == pool;
}
// the handles of the verification calls and of bpgpu_pool_r1cs_prove_fs: a parametric circuit is none of theirs
bool numeric_ok(const bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c) { return handles_ok(pool, g, c) && !c->nchi; }
int shares_of(bpgpu_pool *pool, size_t nb, int option, std::vector<size_t> &lo) {
  int64_t granule = 1;
  if (option) {
    const int rc = bpgpu_get_option(pool->ctx[0], option, &granule);
    if (rc) return rc;
  }
  lo.assign(pool->ctx.size() + 1, 0);
  return bpgpu_pool_shares(nb, pool->ctx.size(), (size_t)granule, lo.data());
}
const uint8_t *at(const uint8_t *p, size_t off) { return p ? p + off : nullptr; }
uint8_t *at(uint8_t *p, size_t off) { return p ? p + off : nullptr; }

// a handle per distinct device, made on the owners' workers at once; all or nothing
template <class Handle>
int make_per_device(bpgpu_pool *pool, std::vector<Handle *> &out, const std::function<int(bpgpu_ctx *, Handle **)> &create,
                    const std::function<void(bpgpu_ctx *, Handle *)> &destroy, const char *what) {
  const size_t ns = pool->ctx.size();
  out.assign(ns, nullptr);
  std::vector<Job> jobs(ns);
  for (size_t s = 0; s < ns; s++)
    if (pool->owner[s] == s) jobs[s] = [&, s]() -> int { return create(pool->ctx[s], &out[s]); };
  const int rc = run_slots(pool, jobs, what);
  if (rc) {
    std::vector<Job> undo(ns);
    for (size_t s = 0; s < ns; s++)
      if (out[s]) undo[s] = [&, s]() -> int { destroy(pool->ctx[s], out[s]); return 0; };
    std::vector<int> codes;
    pool->workers.run(undo, codes);
    out.assign(ns, nullptr);
    return rc;
  }
  for (size_t s = 0; s < ns; s++) out[s] = out[pool->owner[s]];
  return BPGPU_OK;
}
template <class Handle>
void drop_per_device(bpgpu_pool *pool, std::vector<Handle *> &h, const std::function<void(bpgpu_ctx *, Handle *)> &destroy) {
  const size_t ns = pool->ctx.size();
  std::vector<Job> jobs(ns);
  for (size_t s = 0; s < ns && s < h.size(); s++)
    if (pool->owner[s] == s && h[s]) jobs[s] = [&, s]() -> int { destroy(pool->ctx[s], h[s]); return 0; };
  std::vector<int> codes;
  pool->workers.run(jobs, codes);
}
template <class Body> int noexcept_abi(Body body) {
  try { return body(); } catch (const std::bad_alloc &) { return BPGPU_E_OOM; }
}

}  // namespace
#endif
