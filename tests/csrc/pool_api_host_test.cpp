// pool_api_host_test.cpp -- the host logic of the pool (mpc_bulletproof_amd/csrc/bpgpu_pool.hip) on the CPU, against FAKES of the
// single-context entry points and of the four HIP calls it makes: which slot gets which share and which pointers, handles per distinct
// device and their all-or-nothing creation, the option rollback, the refusals that wake nobody, a slot that fails at run time (the
// others finish, the lowest failing slot's code comes back, bpgpu_pool_last_error names it), the 64-byte hand-over of the combined
// check and the in-place rule for page-locked operands.  None of the run-time failures can be staged on a real device.
// tests/test_pool_workers_cpu.py compiles this file together with bpgpu_pool.hip (as host C++) under the thread and the address
// sanitizer and runs both programs.  No GPU and no HIP library: everything the pool calls is defined below.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bpgpu_internal.h"

static int failures = 0;
#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) { failures++; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

// ---- the fakes ------------------------------------------------------------------------------------------------------------------
struct bpgpu_ctx { int device; int id; int64_t opt[BPGPU_OPT_COUNT]; std::string err; };
struct bpgpu_gens { int device; };
struct bpgpu_circuit { int device; };
struct Call { int ctx_id; size_t nb; const void *p0, *p1, *p2, *p3; void *out; int in_place; };

static std::mutex g_mu;
static int g_devices = 0, g_next_id = 0, g_live_ctx = 0, g_live_gens = 0, g_live_circ = 0;
static int g_fail_create_id = -1, g_fail_gens_device = -1, g_refuse_option_id = -1;
static int g_fail_code[64];                 // by context id: what the slot's call returns
static int g_sleep_ms[64];
static std::vector<Call> g_calls;
static const uint8_t *g_pinned_lo = nullptr, *g_pinned_hi = nullptr, *g_pinned_split = nullptr;   // a fake page-locked range of device 0
static thread_local int t_device = -1;
static bpgpu_ctx *g_sum_ctx = nullptr;      // the context the partial points were added on

static void reset_faults() {
  std::lock_guard<std::mutex> lk(g_mu);
  memset(g_fail_code, 0, sizeof g_fail_code);
  memset(g_sleep_ms, 0, sizeof g_sleep_ms);
  g_calls.clear();
}
static int slot_call(bpgpu_ctx *ctx, Call c) {
  EXPECT(t_device == ctx->device);           // issued on the slot's own worker, which selected the device once
  int ms, code;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    c.ctx_id = ctx->id;
    g_calls.push_back(c);
    ms = g_sleep_ms[ctx->id]; code = g_fail_code[ctx->id];
  }
  if (ms) std::this_thread::sleep_for(std::chrono::milliseconds(ms));
  if (code) ctx->err = "fake failure of context " + std::to_string(ctx->id);
  return code;
}

extern "C" {
hipError_t hipSetDevice(int d) { t_device = d; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p) {
  const uint8_t *q = (const uint8_t *)p;
  if (!g_pinned_lo || q < g_pinned_lo || q >= g_pinned_hi) return hipErrorInvalidValue;      // pageable
  memset(a, 0, sizeof *a);
  a->type = hipMemoryTypeHost; a->device = 0; a->devicePointer = (void *)p; a->hostPointer = (void *)p;
  return hipSuccess;
}
hipError_t hipMemGetAddressRange(hipDeviceptr_t *base, size_t *size, hipDeviceptr_t p) {
  const uint8_t *q = (const uint8_t *)p;
  if (!g_pinned_lo || q < g_pinned_lo || q >= g_pinned_hi) return hipErrorInvalidValue;
  const bool second = g_pinned_split && q >= g_pinned_split;                                  // two adjacent allocations
  *base = (hipDeviceptr_t)(second ? g_pinned_split : g_pinned_lo);
  *size = (size_t)(second ? g_pinned_hi - g_pinned_split : (g_pinned_split ? g_pinned_split : g_pinned_hi) - g_pinned_lo);
  return hipSuccess;
}

int bpgpu_device_count(void) { return g_devices; }
const char *bpgpu_strerror(int code) { return code == BPGPU_E_DEVICE ? "device" : code == BPGPU_E_OOM ? "oom" : code == BPGPU_E_LEN ? "len" : "other"; }
const char *bpgpu_last_error(bpgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }
int bpgpu_create(int device, bpgpu_ctx **out) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int id = g_next_id++;
  if (id == g_fail_create_id) return BPGPU_E_OOM;
  *out = new bpgpu_ctx{device, id, {}, ""};
  (*out)->opt[BPGPU_OPT_STREAM_BATCH] = 1024; (*out)->opt[BPGPU_OPT_SCREEN_BATCH] = 2560; (*out)->opt[BPGPU_OPT_STREAM_LANES] = 20;
  g_live_ctx++;
  return BPGPU_OK;
}
void bpgpu_destroy(bpgpu_ctx *ctx) {
  if (!ctx) return;
  std::lock_guard<std::mutex> lk(g_mu);
  g_live_ctx--;
  delete ctx;
}
int bpgpu_get_option(bpgpu_ctx *ctx, int option, int64_t *v) {
  if (!ctx || option <= 0 || option >= BPGPU_OPT_COUNT) return BPGPU_E_ARG;
  *v = ctx->opt[option];
  return BPGPU_OK;
}
int bpgpu_set_option(bpgpu_ctx *ctx, int option, int64_t v) {
  if (!ctx || option <= 0 || option >= BPGPU_OPT_COUNT || v < 0 || ctx->id == g_refuse_option_id) return BPGPU_E_ARG;
  ctx->opt[option] = v;
  return BPGPU_OK;
}
int bpgpu_gens_create(bpgpu_ctx *ctx, const uint8_t *, const uint8_t *, size_t, const uint8_t *, const uint8_t *, int, bpgpu_gens **out) {
  EXPECT(t_device == ctx->device);
  std::lock_guard<std::mutex> lk(g_mu);
  if (ctx->device == g_fail_gens_device) { ctx->err = "no table"; return BPGPU_E_OOM; }
  *out = new bpgpu_gens{ctx->device};
  g_live_gens++;
  return BPGPU_OK;
}
void bpgpu_gens_destroy(bpgpu_ctx *ctx, bpgpu_gens *g) {
  std::lock_guard<std::mutex> lk(g_mu);
  EXPECT(g && ctx->device == g->device);
  g_live_gens--;
  delete g;
}
static int circ_new(bpgpu_ctx *ctx, bpgpu_circuit **out) {
  std::lock_guard<std::mutex> lk(g_mu);
  *out = new bpgpu_circuit{ctx->device};
  g_live_circ++;
  return BPGPU_OK;
}
int bpgpu_circuit_create(bpgpu_ctx *ctx, size_t, const uint32_t *, const uint32_t *, const uint32_t *, const uint8_t *, size_t, size_t,
                         bpgpu_circuit **out) { return circ_new(ctx, out); }
int bpgpu_circuit_create_ark(bpgpu_ctx *ctx, size_t, const uint32_t *, const uint32_t *, const uint32_t *, const uint8_t *, size_t, size_t,
                             bpgpu_circuit **out) { return circ_new(ctx, out); }
void bpgpu_circuit_destroy(bpgpu_ctx *ctx, bpgpu_circuit *c) {
  std::lock_guard<std::mutex> lk(g_mu);
  EXPECT(c && ctx->device == c->device);
  g_live_circ--;
  delete c;
}
int bpgpu_internal_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t, size_t, const uint8_t *points,
                                 const uint8_t *scalars, const uint8_t *challenges, int32_t *ok, int in_place_ok) {
  EXPECT(g->device == ctx->device && c->device == ctx->device);
  const int rc = slot_call(ctx, {0, nb, points, scalars, challenges, nullptr, ok, in_place_ok});
  if (!rc) for (size_t i = 0; i < nb; i++) ok[i] = 100 + ctx->id;
  return rc;
}
int bpgpu_r1cs_verify_screened(bpgpu_ctx *ctx, const bpgpu_gens *, const bpgpu_circuit *, size_t nb, size_t, size_t, const uint8_t *points,
                               const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, int32_t *ok, size_t *fallback_batches) {
  *fallback_batches = (size_t)ctx->id + 1;
  return slot_call(ctx, {0, nb, points, scalars, challenges, rho, ok, -1});
}
int bpgpu_r1cs_verify_combined(bpgpu_ctx *ctx, const bpgpu_gens *, const bpgpu_circuit *, size_t nb, size_t, size_t, const uint8_t *points,
                               const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, uint8_t partial_xy[64]) {
  memset(partial_xy, ctx->id + 1, 64);
  return slot_call(ctx, {0, nb, points, scalars, challenges, rho, partial_xy, -1});
}
int bpgpu_points_sum(bpgpu_ctx *ctx, const uint8_t *points, size_t n, uint8_t out[64]) {
  EXPECT(t_device == ctx->device);
  g_sum_ctx = ctx;
  memset(out, 0, 64);
  for (size_t i = 0; i < n; i++)
    for (int j = 0; j < 64; j++) out[j] = (uint8_t)(out[j] + points[64 * i + j]);
  out[63] = (uint8_t)n;
  return BPGPU_OK;
}
int bpgpu_r1cs_prove_fs(bpgpu_ctx *ctx, const bpgpu_gens *, const bpgpu_circuit *, size_t nb, const uint8_t *states_in, const uint8_t *a_L,
                        const uint8_t *, const uint8_t *, const uint8_t *s_L, const uint8_t *, const uint8_t *vector_keys, const uint8_t *v_blinding,
                        const uint8_t *, uint8_t *proof_points, uint8_t *, uint8_t *wire, uint8_t *, uint8_t *) {
  EXPECT(s_L == nullptr && v_blinding == nullptr);                     // an absent optional operand stays absent in every share
  return slot_call(ctx, {0, nb, states_in, a_L, vector_keys, wire, proof_points, -1});
}
}

static std::vector<Call> calls_by_ctx() {
  std::lock_guard<std::mutex> lk(g_mu);
  std::vector<Call> v(g_calls);
  for (size_t i = 0; i < v.size(); i++)
    for (size_t j = i + 1; j < v.size(); j++)
      if (v[j].ctx_id < v[i].ctx_id) std::swap(v[i], v[j]);
  return v;
}

int main() {
  static uint8_t buf[1 << 20];
  const int devs[3] = {0, 1, 0};
  bpgpu_pool *pool = nullptr;
  // no device: BPGPU_E_DEVICE; then a node of two
  EXPECT(bpgpu_pool_create(devs, 3, &pool) == BPGPU_E_DEVICE && !pool);
  g_devices = 2;
  const int beyond[2] = {0, 2};
  EXPECT(bpgpu_pool_create(beyond, 2, &pool) == BPGPU_E_DEVICE && !pool);
  // a context that cannot be made: the others are released
  g_fail_create_id = g_next_id + 1;
  EXPECT(bpgpu_pool_create(devs, 3, &pool) == BPGPU_E_OOM && !pool && g_live_ctx == 0);
  g_fail_create_id = -1;
  const int id0 = g_next_id;                 // the ids of the three slots (in some order: the workers create concurrently)
  EXPECT(bpgpu_pool_create(devs, 3, &pool) == BPGPU_OK && pool && g_live_ctx == 3);
  EXPECT(bpgpu_pool_slots(pool) == 3 && bpgpu_pool_device(pool, 1) == 1 && bpgpu_pool_device(pool, 3) == BPGPU_E_ARG && !bpgpu_pool_ctx(pool, 3));
  int id[3];
  for (int s = 0; s < 3; s++) { id[s] = bpgpu_pool_ctx(pool, s)->id; EXPECT(id[s] >= id0 && id[s] < id0 + 3 && bpgpu_pool_ctx(pool, s)->device == devs[s]); }

  // handles: one per distinct device, all or nothing
  bpgpu_pool_gens *pg = nullptr;
  g_fail_gens_device = 1;
  EXPECT(bpgpu_pool_gens_create(pool, buf, buf, 8, buf, buf, 8, &pg) == BPGPU_E_OOM && !pg && g_live_gens == 0);
  EXPECT(strstr(bpgpu_pool_last_error(pool), "slot 1 (device 1)") && strstr(bpgpu_pool_last_error(pool), "no table"));
  g_fail_gens_device = -1;
  EXPECT(bpgpu_pool_gens_create(pool, buf, buf, 8, buf, buf, 8, &pg) == BPGPU_OK && pg && g_live_gens == 2);
  EXPECT(bpgpu_pool_gens_get(pg, 0) == bpgpu_pool_gens_get(pg, 2) && bpgpu_pool_gens_get(pg, 0) != bpgpu_pool_gens_get(pg, 1) && !bpgpu_pool_gens_get(pg, 3));
  bpgpu_pool_circuit *pc = nullptr, *pc_ark = nullptr;
  const uint32_t rp[2] = {0, 0};
  EXPECT(bpgpu_pool_circuit_create(pool, 1, rp, rp, rp, buf, 8, 1, &pc) == BPGPU_OK && pc && g_live_circ == 2);
  EXPECT(bpgpu_pool_circuit_create_ark(pool, 1, rp, rp, rp, buf, 8, 1, &pc_ark) == BPGPU_OK && g_live_circ == 4);
  bpgpu_pool_circuit_destroy(pool, pc_ark);
  EXPECT(g_live_circ == 2 && bpgpu_pool_circuit_get(pc, 0) == bpgpu_pool_circuit_get(pc, 2) && bpgpu_pool_circuit_get(pc, 1)->device == 1);

  // options: every slot or none
  EXPECT(bpgpu_pool_set_option(pool, BPGPU_OPT_STREAM_BATCH, 16) == BPGPU_OK && bpgpu_pool_set_option(pool, BPGPU_OPT_SCREEN_BATCH, 16) == BPGPU_OK);
  g_refuse_option_id = id[2];
  EXPECT(bpgpu_pool_set_option(pool, BPGPU_OPT_STREAM_BATCH, 64) == BPGPU_E_ARG);
  g_refuse_option_id = -1;
  for (int s = 0; s < 3; s++) EXPECT(bpgpu_pool_ctx(pool, s)->opt[BPGPU_OPT_STREAM_BATCH] == 16);
  EXPECT(bpgpu_pool_set_option(pool, BPGPU_OPT_STREAM_BATCH, -1) == BPGPU_E_ARG && bpgpu_pool_ctx(pool, 0)->opt[BPGPU_OPT_STREAM_BATCH] == 16);

  // the stream call: 150 proofs in granules of 16 -> 64 | 48 | 38; n = 8 multipliers, m = 1, k = 3: 18 points, 5 scalars, 9 challenges
  const size_t nb = 150, k = 3, bp = 18 * 64, bs = 160, bc = 9 * 32;
  uint8_t *P = buf, *S = buf + 300000, *Cc = buf + 400000, *R = buf + 500000;
  static int32_t ok[150];
  size_t per[3] = {9, 9, 9};
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_OK);
  EXPECT(per[0] == 64 && per[1] == 48 && per[2] == 38);
  const size_t lo[4] = {0, 64, 112, 150};
  for (int s = 0; s < 3; s++) {
    bool found = false;
    for (const Call &c : calls_by_ctx())
      if (c.ctx_id == id[s]) {
        found = true;
        EXPECT(c.nb == lo[s + 1] - lo[s] && c.p0 == P + lo[s] * bp && c.p1 == S + lo[s] * bs && c.p2 == Cc + lo[s] * bc && c.out == ok + lo[s]);
        EXPECT(c.in_place == 0);             // pageable operands: staged copies
      }
    EXPECT(found);
    for (size_t i = lo[s]; i < lo[s + 1]; i++) EXPECT(ok[i] == 100 + id[s]);
  }
  // five proofs: one granule, two slots are not woken; no proof: nothing is touched
  reset_faults();
  per[0] = per[1] = per[2] = 9;
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, 5, 8, k, P, S, Cc, ok, per) == BPGPU_OK && per[0] == 5 && per[1] == 0 && per[2] == 0);
  EXPECT(calls_by_ctx().size() == 1 && calls_by_ctx()[0].ctx_id == id[0]);
  reset_faults();
  per[0] = 9;
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, 0, 8, k, nullptr, nullptr, nullptr, nullptr, per) == BPGPU_OK && per[0] == 9 && calls_by_ctx().empty());

  // refusals wake nobody: shapes, null operands, handles of another pool
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, 32, P, S, Cc, ok, per) == BPGPU_E_LEN);
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 9, k, P, S, Cc, ok, per) == BPGPU_E_LEN);       // n1 > n
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, 2, P, S, Cc, ok, per) == BPGPU_E_LEN);       // n > 2^k
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, nullptr, Cc, ok, per) == BPGPU_E_ARG);
  EXPECT(bpgpu_pool_r1cs_verify_combined(pool, pg, pc, nb, 8, k, P, S, Cc, R, nullptr) == BPGPU_E_ARG);
  bpgpu_pool_gens *small = nullptr;
  EXPECT(bpgpu_pool_gens_create(pool, buf, buf, 4, buf, buf, 8, &small) == BPGPU_OK);
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, small, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_E_GENS);
  EXPECT(bpgpu_pool_r1cs_prove_fs(pool, small, pc, 7, P, P, P, P, nullptr, nullptr, P, nullptr, P, P, P, nullptr, nullptr, nullptr) == BPGPU_E_GENS);
  bpgpu_pool_gens_destroy(pool, small);
  const int one[1] = {0};
  bpgpu_pool *other = nullptr;
  EXPECT(bpgpu_pool_create(one, 1, &other) == BPGPU_OK);
  EXPECT(bpgpu_pool_r1cs_verify_stream(other, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_E_ARG);
  bpgpu_pool_destroy(other);
  EXPECT(calls_by_ctx().empty() && g_live_ctx == 3 && g_live_gens == 2);

  // a slot fails at run time: the others finish (slot 0 is the slowest), the LOWEST failing slot's code comes back
  reset_faults();
  g_sleep_ms[id[0]] = 30; g_fail_code[id[1]] = BPGPU_E_DEVICE; g_fail_code[id[2]] = BPGPU_E_OOM;
  memset(ok, 0, sizeof ok);
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_E_DEVICE);
  EXPECT(calls_by_ctx().size() == 3 && ok[0] == 100 + id[0] && ok[63] == 100 + id[0] && ok[64] == 0);
  const std::string msg = bpgpu_pool_last_error(pool);
  EXPECT(msg.find("slot 1 (device 1)") != std::string::npos && msg.find("fake failure of context " + std::to_string(id[1])) != std::string::npos);
  reset_faults();
  g_fail_code[id[2]] = BPGPU_E_OOM;
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_E_OOM);
  EXPECT(strstr(bpgpu_pool_last_error(pool), "slot 2 (device 0)"));
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_OK);        // and the pool goes on working

  // screened: the shares of BPGPU_OPT_SCREEN_BATCH, the weights sliced, the fallback batches summed
  reset_faults();
  size_t nf = 0;
  EXPECT(bpgpu_pool_r1cs_verify_screened(pool, pg, pc, nb, 8, k, P, S, Cc, R, ok, &nf) == BPGPU_OK);
  EXPECT(nf == (size_t)(id[0] + id[1] + id[2] + 3));
  for (const Call &c : calls_by_ctx())
    for (int s = 0; s < 3; s++)
      if (c.ctx_id == id[s]) EXPECT(c.nb == lo[s + 1] - lo[s] && c.p0 == P + lo[s] * bp && c.p3 == R + lo[s] * 32 && c.out == ok + lo[s]);

  // combined: one partial per NON-EMPTY slot, added on slot 0 (the fake sum adds bytes and leaves the count in byte 63)
  uint8_t xy[64];
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_combined(pool, pg, pc, nb, 8, k, P, S, Cc, R, xy) == BPGPU_OK);
  EXPECT(g_sum_ctx == bpgpu_pool_ctx(pool, 0) && xy[63] == 3 && xy[0] == id[0] + id[1] + id[2] + 3 && calls_by_ctx().size() == 3);
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_combined(pool, pg, pc, 5, 8, k, P, S, Cc, R, xy) == BPGPU_OK && xy[63] == 1 && xy[0] == id[0] + 1);
  reset_faults();
  g_fail_code[id[1]] = BPGPU_E_ARG;          // a malformed operand in the middle share fails the call, as on one context
  g_sum_ctx = nullptr;
  EXPECT(bpgpu_pool_r1cs_verify_combined(pool, pg, pc, nb, 8, k, P, S, Cc, R, xy) == BPGPU_E_ARG && !g_sum_ctx);

  // the in-place rule: only a slot whose device owns its whole share, inside ONE allocation, reads page-locked operands in place
  EXPECT(bpgpu_pool_set_option(pool, BPGPU_OPT_STREAM_BATCH, 75) == BPGPU_OK);      // shares 75 | 75 | 0
  g_pinned_lo = buf; g_pinned_hi = buf + sizeof buf;                                  // everything page-locked under device 0
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_OK && per[0] == 75 && per[1] == 75 && per[2] == 0);
  for (const Call &c : calls_by_ctx()) EXPECT(c.in_place == (c.ctx_id == id[0] ? 1 : 0));        // slot 1 sits on device 1
  g_pinned_split = P + 10 * bp;                                                       // slot 0's points straddle two allocations
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_OK);
  for (const Call &c : calls_by_ctx()) EXPECT(c.in_place == 0);
  g_pinned_split = nullptr;
  g_pinned_hi = Cc + 10;                                                              // the challenges are pageable
  reset_faults();
  EXPECT(bpgpu_pool_r1cs_verify_stream(pool, pg, pc, nb, 8, k, P, S, Cc, ok, per) == BPGPU_OK);
  for (const Call &c : calls_by_ctx()) EXPECT(c.in_place == 0);
  g_pinned_lo = g_pinned_hi = nullptr;

  // the prover: granule 1 -> 3 | 2 | 2 of seven provers; absent optional operands stay absent, present ones are sliced
  reset_faults();
  const size_t plo[4] = {0, 3, 5, 7};
  EXPECT(bpgpu_pool_r1cs_prove_fs(pool, pg, pc, 7, P, S, S, S, nullptr, nullptr, Cc, nullptr, R, buf + 600000, buf + 700000, nullptr, nullptr, nullptr) ==
         BPGPU_E_ARG);                       // m = 1 and no v_blinding: refused, nobody woken
  EXPECT(calls_by_ctx().empty());
  bpgpu_pool_circuit *pc0 = nullptr;         // the same without commitments
  EXPECT(bpgpu_pool_circuit_create(pool, 1, rp, rp, rp, buf, 8, 0, &pc0) == BPGPU_OK);
  EXPECT(bpgpu_pool_r1cs_prove_fs(pool, pg, pc0, 7, P, S, S, S, nullptr, nullptr, Cc, nullptr, R, buf + 600000, buf + 700000, nullptr, nullptr, nullptr) ==
         BPGPU_OK);
  for (const Call &c : calls_by_ctx())
    for (int s = 0; s < 3; s++)
      if (c.ctx_id == id[s])
        EXPECT(c.nb == plo[s + 1] - plo[s] && c.p0 == P + plo[s] * 32 && c.p1 == S + plo[s] * 8 * 32 && c.p2 == Cc + plo[s] * 32 && c.p3 == nullptr &&
               c.out == buf + 600000 + plo[s] * (11 + 2 * 3) * 64);
  EXPECT(calls_by_ctx().size() == 3);
  EXPECT(bpgpu_pool_r1cs_prove_fs(pool, pg, pc0, 7, P, S, S, S, S, S, Cc, nullptr, R, buf, buf, nullptr, nullptr, nullptr) == BPGPU_E_ARG);   // both sources
  bpgpu_pool_circuit_destroy(pool, pc0);
  bpgpu_pool_circuit_destroy(pool, pc);
  bpgpu_pool_gens_destroy(pool, pg);
  EXPECT(g_live_gens == 0 && g_live_circ == 0);
  bpgpu_pool_destroy(pool);
  EXPECT(g_live_ctx == 0);
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("all passed\n");
  return 0;
}
