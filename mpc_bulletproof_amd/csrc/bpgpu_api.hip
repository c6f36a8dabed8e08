// bpgpu_api.hip -- the C ABI of include/bpgpu.h on top of the HIP kernels.
// No CPU fallback: every entry point needs a live HIP device and fails with BPGPU_E_DEVICE otherwise.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/bpgpu.h"
#include "kernels.h"
#include "bpgpu_internal.h"
#include "fe29.cuh"
#include "queue_plan.h"

using namespace bpk;

namespace {

struct Slot { void *p = nullptr; size_t cap = 0; };

// Workspace slots (bpgpu_ctx::ws), one grow-only device buffer each.  ws_get may free and reallocate a slot, so no function ws_gets
// a slot that one of its callers still holds.  (verify_plan takes the "verifier:" slots, WS_ZPOW and WS_STRAUS on behalf of
// verify_batch_dev_locked; the launch routes under it take WS_MSM, WS_MSM2 and msm_wp_batch's.)
enum WsSlot : int {
  // an entry point's operands, results and small scratch (host staging, a lane's batch); the cores below an entry point take the
  // ones it leaves free (msm_batch_dev_locked: 2-4 under msm_batch_locked's 0, 1, 5; verify_wire_locked: 0-2 under the host form's 3-5;
  // session_polys_begin: 0 for z, besides WS_CHI).  The helpers of the variable-base MSMs and of the polynomial build take none of
  // these: msm_tail WS_PIP or WS_STRAUS, zpow_build WS_ZPOW.
  WS_ARG0, WS_ARG1, WS_ARG2, WS_ARG3, WS_ARG4, WS_ARG5,
  WS_ZPOW,          // z-power tables: flatten, prover polynomials, the verifier's scalar assembly
  WS_VPTS,          // verifier: converted proof points
  WS_VFIX,          // verifier: generator-half scalars; bpgpu_msm_shared: point replicas
  WS_VVAR,          // verifier: proof-point scalars
  WS_VVRES,         // verifier: proof-point sums; combined check: weighted generator column sums
  WS_VFRES,         // verifier: generator-half sums; combined check: the two halves
  WS_MSM,           // window-parallel scratch, fixed-base chunk partials (msm_gens_dev), second Straus scratch, msm_core_locked's terms
  WS_STRAUS,        // Straus tables (straus_ws)
  WS_PIP,           // bucket-method and combined-check pipelines (k_pip.hip, k_pip2.hip; k_mixed.hip: mixed_run_locked)
  WS_VAUX,          // wire format / decode bits (verify_wire_locked, wire_front_locked); combined check: final sum
  WS_FS_STAGE,      // transcript host forms: challenges out, wire verdicts; bpgpu_ipp_run_fs: transcript states
  WS_FS_CH,         // device transcript: challenges; bpgpu_ipp_run_fs: L, R
  WS_PROOF_BAD,     // per-proof rejects: transcript identity points, non-canonical gadget challenges; bpgpu_ipp_run_fs: zero flag
  WS_SCHED,         // device transcript schedule (bpgpu_ctx::sched_key)
  WS_VBITS,         // verifier: per-proof malformed scalar | point bits (bpgpu_r1cs_verify_shard gets the same buffer before it calls in)
  WS_CHI,           // gadget challenges: uploaded, or derived by the device transcript
  WS_CHI_OUT,       // bpgpu_r1cs_verify_batch_fs(2): gadget challenges out
  WS_MSM2,          // fixed-base chunk partials under a caller that holds WS_MSM (verifier); two-party masked and opened values
  WS_WP_PTS,        // msm_wp_batch: padded points
  WS_WP_SC,         // msm_wp_batch: padded scalars
  WS_SCREEN_PART,   // screened calls (screen_locked): one partial point per check; queue_combined_locked: the checks' partials
  WS_SCREEN_FLAG,   // screened calls (screen_locked): one input flag per check; queue_combined_locked: the partials' sum flag
  WS_WP_RED,        // msm_wp_batch: scratch of the reduced instances
  WS_MIXED_STAGE,   // mixed host forms (queue_stage_locked): every group's operands and verdicts
  WS_IPPV_STAGE,    // bpgpu_ipp_verify_*: the host forms' operands and results
  WS_IPPV_HDR,      // ... per-proof header values, reject marks
  WS_IPPV_SC,       // ... MSM scalars: dense instances, or the generator half over resident generators
  WS_IPPV_VSC,      // ... resident generators: the scalars of L, R
  WS_IPPV_PTS,      // ... converted points in instance layout
  WS_IPPV_SUM,      // ... MSM sums, expect_P when the caller does not ask for it
  WS_PFS_STAGE,     // bpgpu_r1cs_prove_fs: the host form's operands and results
  WS_PFS_CH,        // ... chain states, the challenge arrays y z u x w u_1..u_k
  WS_PFS_SC,        // ... blindings and v_blinding (plain), T rows, tb2, t_x t_x_blinding e_blinding
  WS_PFS_PTS,       // ... A_I A_O S and T_1..T_6: sums and boundary bytes
  WS_PFS_SCHED,     // ... the prover's transcript schedule (bpgpu_ctx::psched[0])
  WS_PFS_SCHED2,    // bpgpu_r1cs_prove_fs2_begin / _finish: the two-phase schedule (bpgpu_ctx::psched[1])
  WS_WIRE_SCHED,    // wire_schedules_locked (WireQueue::prepare): the transcript schedules of a call's groups (on the calling context; the lanes read it)
  WS_COUNT
};

}  // namespace

struct bpgpu_ctx {
  int device = 0;
  hipStream_t st = nullptr, st2 = nullptr;
  hipEvent_t ev1 = nullptr, ev2 = nullptr;
  std::mutex mu;
  std::string err;
  int *d_flag = nullptr;          // device int: bad-input flag
  void *sqrt_tab = nullptr;       // F_p square-root tables of the point codec (built on first use)
  struct bpgpu_gens *gen_tab = nullptr;   // 16-bit-window table of the curve generator (bpgpu_generator_mul)
  Slot ws[WS_COUNT];              // grow-only workspace slots
  // optional per-kernel HIP-event timing (bench.py roofline): kind -> list of (start, stop)
  bool prof = false;
  bool latency_mode = false;      // bpgpu_set_latency_mode
  int horner_group = 0;           // bpgpu_set_horner_group: windows per group of the first Horner stage, 0 = by mode
  size_t shard_rank = 0, shard_world = 1;   // bpgpu_set_shard: this context's share of ONE large proof split over the GPUs of a node
  // bpgpu_set_option: launch-route selectors of THIS context (tests walk every route through them; a multi-tenant host gives
  // each tenant its own context).  The BPGPU_* environment variables of the same names only seed the defaults, once, in bpgpu_create.
  int64_t opt[BPGPU_OPT_COUNT] = {};
  std::vector<hipEvent_t> prof_ev[BPGPU_PROF_KINDS];
  std::vector<hipEvent_t> prof_pool;   // recycled events
  std::vector<hipEvent_t> prof_epochs; // reference events handed out by bpgpu_profile_epoch (alive as long as the context)
  bool prof_skip[BPGPU_PROF_KINDS] = {};
  uint32_t prof_mask = 0xffffffffu;    // bpgpu_profile_select
  // Device buffers of the prover / IPP sessions, recycled between sessions: hipFree waits for the WHOLE device to idle, which
  // serialises two contexts that pipeline batches (one host thread each), and a session is a dozen allocations.
  struct PoolBlk { void *p; size_t cap; bool used; };
  std::vector<PoolBlk> pool;
  // bpgpu_r1cs_verify_stream: the ring of lanes (child contexts: one stream + workspaces each) this context spreads the batches
  // of one call over; created on first use, owned by the parent
  std::vector<bpgpu_ctx *> lanes;
  hipEvent_t lane_ev = nullptr;   // fork / join marker of a stream call
  void *pinned = nullptr;         // page-locked staging for the verdicts of a host-memory stream or screened call (pinned_verdicts)
  size_t pinned_cap = 0;
  // device-transcript schedule cache (m, k, padded_n) -> steps already resident in WS_SCHED
  size_t sched_key[4] = {(size_t)-1, (size_t)-1, (size_t)-1, 0};   // m, k, padded n + (nchi << 40), the circuit's labels_id (0: none)
  int sched_len = 0;
  // the prover's schedules (prover_schedule), [0] of bpgpu_r1cs_prove_fs in WS_PFS_SCHED, [1] of bpgpu_r1cs_prove_fs2_begin / _finish in
  // WS_PFS_SCHED2: (m, padded_n, nchi, the circuit's labels_id or 0) -> steps resident (and the label table behind them), and their
  // three / four slices
  struct { size_t key[4] = {(size_t)-1, (size_t)-1, 0, 0}; int cut[5] = {0, 0, 0, 0, 0}; } psched[2];
  // bpgpu_r1cs_verify_mixed_wire_*: page-locked staging of a call's schedules and the mark of its upload (the next call waits for
  // the mark before it refills the staging -- passed long before, except when _dev calls follow each other without a bpgpu_sync)
  void *wsched_host = nullptr;
  size_t wsched_cap = 0;
  hipEvent_t wsched_ev = nullptr;
};
struct ProfScope {   // records start/stop events on `st` around a launch when profiling is on (events come from a per-context pool)
  bpgpu_ctx *c; int kind; hipStream_t st;
  // start and stop marks of a kind alternate (scopes of one kind do not nest).  At most PROF_CAP timed launches per kind are
  // kept between two reads: a long run samples its first launches instead of creating thousands of events inside the timed
  // region (2 048 steps: 1 200 hipEventCreate calls on the sampled context cost the run 5 % of its throughput).
  static constexpr size_t PROF_CAP = 256;
  static void mark(bpgpu_ctx *c, int kind, hipStream_t st) {
    auto &v = c->prof_ev[kind];
    if (!((c->prof_mask >> kind) & 1u)) return;
    if (c->prof_skip[kind]) { c->prof_skip[kind] = false; return; }                       // the stop of a skipped start
    if ((v.size() & 1) == 0 && v.size() >= 2 * PROF_CAP) { c->prof_skip[kind] = true; return; }
    hipEvent_t e = nullptr;
    if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); }
    else if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    c->prof_ev[kind].push_back(e);
  }
  ProfScope(bpgpu_ctx *c_, int kind_, hipStream_t st_) : c(c_), kind(kind_), st(st_) { if (c->prof) mark(c, kind, st); }
  ~ProfScope() { if (c->prof) mark(c, kind, st); }
};
// the same with an explicit end: entry points that wait for their results close the span BEFORE the host-side wait (error paths
// close it on the way out)
struct ProfSpan {
  bpgpu_ctx *c; int kind; hipStream_t st; bool open;
  ProfSpan(bpgpu_ctx *c_, int kind_, hipStream_t st_) : c(c_), kind(kind_), st(st_), open(c_->prof) { if (open) ProfScope::mark(c, kind, st); }
  void close() { if (open) { ProfScope::mark(c, kind, st); open = false; } }
  ~ProfSpan() { close(); }
};
static void prof_mark_cb(void *c, int kind, hipStream_t st) { ProfScope::mark((bpgpu_ctx *)c, kind, st); }
struct bpgpu_gens {
  size_t cap = 0;
  int c = 0;
  AffDev *points = nullptr;       // [B, B_blinding, G_0..G_{cap-1}, H_0..H_{cap-1}]
  AffDev *table = nullptr;        // (2 + 2 cap) * W * 2^(c-1)
};
// lock-step InnerProductProof::create state for nb proofs (device resident between rounds)
struct bpgpu_ipp {
  size_t nb = 0, n0 = 0, n = 0;
  bool first = true, shared_gens = false;
  Words8 *a[2] = {nullptr, nullptr}, *b[2] = {nullptr, nullptr};   // ping-pong, nb x n
  AffDev *G[2] = {nullptr, nullptr}, *H[2] = {nullptr, nullptr};   // [0]: input (n0 or nb x n0), [1]/[0] folded
  AffDev *Q = nullptr;
  Words8 *Gf = nullptr, *Hf = nullptr;                             // nb x n0 (first round only)
  Words8 *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *t4 = nullptr;   // nb x n0/2 temporaries
  Words8 *cLR = nullptr, *uu = nullptr;                            // nb x 2 each (uu: u | u_inv as 2 arrays of nb)
  JacRaw *res = nullptr, *sums = nullptr;                          // nb x 2 x (n0 + 1), nb x 2
  AffDev *mpts = nullptr;                                          // nb x 2 x (n0 + 1): contiguous MSM operands
  Words8 *msc = nullptr;                                           //   (bucket-method rounds)
  Words8 *out_xy = nullptr;                                        // nb x 2 points
  const JacRaw *tail_partials = nullptr;                           // the last round MSM's chunk partials, when the fused round tail sums them
  size_t tail_chunks = 0;
  int cur = 0;                                                     // index of the live a/b/G/H buffers
  bpgpu_gens *own_gens = nullptr;                                  // tables built for this session only (bpgpu_ipp_begin, one proof)
  const bpgpu_gens *gens = nullptr;                                // resident-generator mode: no G/H buffers,
  Words8 *cG = nullptr, *cH = nullptr, *w = nullptr;               //   coefficient vectors nb x n0 and Q = w * B
  size_t slo = 0, shi = (size_t)-1;                                // bpgpu_set_shard at session start: the generators whose terms this
  bool with_q = true;                                              //   rank's L, R carry (the c Q term belongs to rank 0)
  int planes = 1;                                                  // 3: authenticated session of bpgpu_mpc_prover_ipp_begin (nb = 3 x proofs)
  Words8 *trip = nullptr;                                          //   its round's Beaver triples (bpgpu_mpc_ipp_mask -> _round)
  bool masked = false;
};
struct bpgpu_circuit {
  size_t q = 0, n = 0, m = 0, nnz = 0, nchi = 0;   // nchi: gadget challenges the coefficients are affine in (kernels.h CircuitDev)
  uint32_t *col_ptr = nullptr, *row = nullptr;
  Words8 *coeff = nullptr;
  // bpgpu_circuit_set_gadget_labels: the nchi labels of the gadgets' challenge_scalar calls in draw order (nchi x 32 B, host memory;
  // empty: none attached, the device-transcript calls take the one label as an argument).  labels_id is unique over the process
  // and changes with every attachment: the contexts' resident schedules (with the label table behind the steps) are keyed by it.
  std::vector<uint8_t> labels;
  uint64_t labels_id = 0;
  // the row-major view (kernels.h RowsDev), built by the first bpgpu_r1cs_constraints_satisfied / bpgpu_mpc_constraints_eval that sees
  // the handle and kept until bpgpu_circuit_destroy.  A handle serves several contexts of a device, each with its own mutex: view_mu
  // guards the one-time build (taken with the calling context's mutex held, never the other way round).
  mutable std::mutex view_mu;
  mutable void *view_mem = nullptr;
  mutable RowsDev view{};
  mutable bool view_ready = false;
};

#define HIPCK(ctx, call)                                                                    \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess) {                                                                \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                      \
      return e__ == hipErrorOutOfMemory ? BPGPU_E_OOM : BPGPU_E_DEVICE;                     \
    }                                                                                       \
  } while (0)
#define CK(x)                \
  do {                       \
    int rc__ = (x);          \
    if (rc__ != BPGPU_OK) return rc__; \
  } while (0)

// session buffers (ctx->mu held): best fit among the free blocks of at most twice the size, else a new allocation; released blocks
// stay with the context (at most 48 free ones: beyond that the largest goes back to the device)
static bool pool_alloc(bpgpu_ctx *ctx, void **out, size_t bytes) {
  *out = nullptr;
  bytes = (bytes + 255) & ~(size_t)255;
  if (!bytes) bytes = 256;
  int best = -1;
  for (size_t i = 0; i < ctx->pool.size(); i++) {
    auto &b = ctx->pool[i];
    if (!b.used && b.cap >= bytes && b.cap <= 2 * bytes + 4096 && (best < 0 || b.cap < ctx->pool[best].cap)) best = (int)i;
  }
  if (best >= 0) { ctx->pool[best].used = true; *out = ctx->pool[best].p; return true; }
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {   // give the cached blocks back and try once more
    for (auto &b : ctx->pool) if (!b.used && b.p) { (void)hipFree(b.p); b.p = nullptr; }
    std::vector<bpgpu_ctx::PoolBlk> keep;
    for (auto &b : ctx->pool) if (b.p) keep.push_back(b);
    ctx->pool.swap(keep);
    if (hipMalloc(&p, bytes) != hipSuccess) return false;
  }
  try { ctx->pool.push_back({p, bytes, true}); } catch (const std::bad_alloc &) { (void)hipFree(p); return false; }
  *out = p;
  return true;
}
static void pool_release(bpgpu_ctx *ctx, void *p) {
  if (!p) return;
  size_t nfree = 0, largest = (size_t)-1;
  for (size_t i = 0; i < ctx->pool.size(); i++) {
    auto &b = ctx->pool[i];
    if (b.p == p) b.used = false;
    if (!b.used) { nfree++; if (largest == (size_t)-1 || b.cap > ctx->pool[largest].cap) largest = i; }
  }
  if (nfree > 48 && largest != (size_t)-1) {
    (void)hipFree(ctx->pool[largest].p);
    ctx->pool.erase(ctx->pool.begin() + (long)largest);
  }
}
// the buffers of a session under construction, one after the other: the first failure sticks, and the session's owner gives back
// what was taken (slot: the address of a device pointer of the session)
struct PoolTake {
  bpgpu_ctx *ctx;
  bool ok = true;
  template <class T> void operator()(T **slot, size_t bytes) { ok = ok && pool_alloc(ctx, (void **)slot, bytes); }
};
// No exception crosses the C ABI: an entry point that stages on the host (std::vector) runs its body in here, and an allocation
// that fails is BPGPU_E_OOM.
template <class Body> static int noexcept_abi(Body body) {
  try { return body(); } catch (const std::bad_alloc &) { return BPGPU_E_OOM; }
}
static int ws_get(bpgpu_ctx *ctx, WsSlot slot, size_t bytes, void **out) {
  Slot &s = ctx->ws[slot];
  if (bytes < 256) bytes = 256;
  if (s.cap < bytes) {
    if (s.p) { HIPCK(ctx, hipStreamSynchronize(ctx->st)); HIPCK(ctx, hipStreamSynchronize(ctx->st2)); HIPCK(ctx, hipFree(s.p)); s.p = nullptr; s.cap = 0; }
    size_t want = bytes + bytes / 4;
    HIPCK(ctx, hipMalloc(&s.p, want));
    s.cap = want;
  }
  *out = s.p;
  return BPGPU_OK;
}
// scratch for the per-lane Straus tables; launches on ctx->st are in order, so they share it
static int straus_ws(bpgpu_ctx *ctx, int np, size_t n, void **out) { return ws_get(ctx, WS_STRAUS, straus_scratch_bytes(np, n), out); }
static int flag_reset(bpgpu_ctx *ctx) { HIPCK(ctx, hipMemsetAsync(ctx->d_flag, 0, sizeof(int), ctx->st)); return BPGPU_OK; }
static int flag_read(bpgpu_ctx *ctx, int *v) {
  HIPCK(ctx, hipMemcpyAsync(v, ctx->d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
// (n == 0 copies nothing and touches neither pointer: the upload / download lists below pass an absent optional operand that way)
static int h2d(bpgpu_ctx *ctx, void *d, const void *h, size_t n) {
  if (n) HIPCK(ctx, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->st));
  return BPGPU_OK;
}
static int d2h(bpgpu_ctx *ctx, void *h, const void *d, size_t n) {
  if (n) HIPCK(ctx, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->st));
  return BPGPU_OK;
}
// an operand of a core that serves host forms and device forms alike: uploaded, or copied within HBM (stream-ordered either way)
static int copy_in(bpgpu_ctx *ctx, void *d, const void *src, size_t n, bool src_dev) {
  if (n) HIPCK(ctx, hipMemcpyAsync(d, src, n, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->st));
  return BPGPU_OK;
}
static int launch_ok(bpgpu_ctx *ctx) { HIPCK(ctx, hipGetLastError()); return BPGPU_OK; }
// Work on the context's second stream beside ctx->st: side_fork (st2 waits for what st holds so far), the launches on st2, side_done
// (marks the end of st2's part), more launches on st, side_join (st waits for the mark)
static int side_fork(bpgpu_ctx *ctx) {
  HIPCK(ctx, hipEventRecord(ctx->ev1, ctx->st));
  HIPCK(ctx, hipStreamWaitEvent(ctx->st2, ctx->ev1, 0));
  return BPGPU_OK;
}
static int side_done(bpgpu_ctx *ctx) { HIPCK(ctx, hipEventRecord(ctx->ev2, ctx->st2)); return BPGPU_OK; }
static int side_join(bpgpu_ctx *ctx) { HIPCK(ctx, hipStreamWaitEvent(ctx->st, ctx->ev2, 0)); return BPGPU_OK; }
// the head of an entry point whose launches validate into ctx->d_flag: the flag cleared, then the operands' uploads in order.
// Where the operands come from: host memory (the staged entry points) or HBM (src_dev: the one-call prover chains the same cores
// on challenges its transcript kernel has just written, and keeps ONE flag for the whole chain: reset = false).
struct OperandSrc { bool src_dev = false, reset = true; };
struct H2D { void *dev; const void *host; size_t bytes; };
static int upload_inputs(bpgpu_ctx *ctx, std::initializer_list<H2D> ins, OperandSrc from = {}) {
  if (from.reset) CK(flag_reset(ctx));
  for (const H2D &i : ins) CK(copy_in(ctx, i.dev, i.host, i.bytes, from.src_dev));
  return BPGPU_OK;
}
// the end of the uploads of an entry point whose launches validate into ctx->d_flag: the launch check, the flag (a host-side wait),
// BPGPU_E_ARG when it is raised
static int checked_inputs(bpgpu_ctx *ctx) {
  CK(launch_ok(ctx));
  int bad = 0;
  CK(flag_read(ctx, &bad));
  return bad ? BPGPU_E_ARG : BPGPU_OK;
}
// the same at the end of an entry point, before anything is downloaded; then the downloads and the wait for them
struct D2H { void *host; const void *dev; size_t bytes; };
static int checked_download(bpgpu_ctx *ctx, std::initializer_list<D2H> outs) {
  CK(checked_inputs(ctx));
  for (const D2H &o : outs) CK(d2h(ctx, o.host, o.dev, o.bytes));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
// rounds x count pairs of points (64 B each: the L, R of IPP rounds, a session's folded G', H'), interleaved and round-major in HBM, into
// two host arrays, item-major: out0[i][r], out1[i][r].  `also` are downloads that ride on the same wait.
static int download_pairs(bpgpu_ctx *ctx, const void *dev, size_t count, size_t rounds, uint8_t *out0, uint8_t *out1,
                          std::initializer_list<D2H> also = {}) {
  std::vector<uint8_t> tmp(rounds * count * 128);
  CK(d2h(ctx, tmp.data(), dev, tmp.size()));
  for (const D2H &o : also) CK(d2h(ctx, o.host, o.dev, o.bytes));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  for (size_t i = 0; i < count; i++)
    for (size_t r = 0; r < rounds; r++) {
      memcpy(out0 + (i * rounds + r) * 64, &tmp[(r * count + i) * 128], 64);
      memcpy(out1 + (i * rounds + r) * 64, &tmp[(r * count + i) * 128 + 64], 64);
    }
  return BPGPU_OK;
}
// One launch that brings a batch's three operand arrays from page-locked host memory into the lane's buffers: wide, coalesced reads
// over the bus by 256 waves (no DMA command, no cross-engine dependency), so that the chain's latency-bound kernels -- the table
// lanes, the scalar assembly -- read HBM, not the bus.  Sizes in 16-byte words.
__global__ void __launch_bounds__(256) k_fetch3(const uint4 *s0, uint4 *d0, size_t n0, const uint4 *s1, uint4 *d1, size_t n1,
                                                const uint4 *s2, uint4 *d2, size_t n2) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1 + n2; i += stride) {
    if (i < n0) d0[i] = s0[i];
    else if (i < n0 + n1) d1[i - n0] = s1[i - n0];
    else d2[i - n0 - n1] = s2[i - n0 - n1];
  }
}
// the device-side address of a page-locked (device-mapped) host allocation, or nullptr for pageable / unknown memory
static const void *host_device_alias(const void *h) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, h) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
  return a.devicePointer;
}

// ---- small device helpers that live with the API ------------------------------------------------
__global__ void k_coeff_to_mont(Words8 *io, size_t n, int *bad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int j = 0; j < 8; j++) w[j] = io[i].w[j];
  if (!bp::words_lt_mod<bp::FN>(w)) { atomicOr(bad, 1); return; }
  bp::Fn x = bp::canon(bp::to_mont(bp::unpack<bp::FN>(w)));
  bp::pack(w, x);
  for (int j = 0; j < 8; j++) io[i].w[j] = w[j];
}
// the same from ark-ff Montgomery limbs (x 2^256 mod n): one multiplication by 2^266 instead of the host's de-Montgomery
__global__ void k_coeff_ark_to_mont(Words8 *io, size_t n, int *bad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int j = 0; j < 8; j++) w[j] = io[i].w[j];
  if (!bp::words_lt_mod<bp::FN>(w)) { atomicOr(bad, 1); return; }
  constexpr int32_t C[bp::NL] = FN_ARK_MONT;
  bp::Fn k;
  for (int j = 0; j < bp::NL; j++) k.v[j] = C[j];
  bp::Fn x = bp::canon(bp::mul(bp::unpack<bp::FN>(w), k));
  bp::pack(w, x);
  for (int j = 0; j < 8; j++) io[i].w[j] = w[j];
}
static int msm_gens_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint32_t *dsc, JacRaw *dres,
                        hipStream_t st, WsSlot part_slot = WS_MSM, int lpm = 0, int kinds = 0) {
  size_t chunks = fixed_msm_chunks(g->c, n, nb, kinds);
  void *dpart = nullptr;
  if (chunks > 1) CK(ws_get(ctx, part_slot, nb * chunks * sizeof(JacRaw), &dpart));
  fixed_msm(st, g->c, g->table, n, g->cap, dsc, (2 + 2 * n) * 8, dres, nb, (JacRaw *)dpart, lpm, kinds);
  return BPGPU_OK;
}

extern "C" {
#pragma GCC visibility push(default)

int bpgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
const char *bpgpu_strerror(int code) {
  switch (code) {
    case BPGPU_OK: return "ok";
    case BPGPU_E_ARG: return "malformed argument (non-canonical scalar, off-curve point, null pointer)";
    case BPGPU_E_LEN: return "length mismatch";
    case BPGPU_E_DEVICE: return "HIP device error (no CPU fallback exists)";
    case BPGPU_E_OOM: return "out of device memory";
    case BPGPU_E_GENS: return "generator capacity too small";
    default: return "unknown";
  }
}
// The pipelined entry points keep ~20 kernels' worth of independent batches in flight, one stream each; the HIP runtime maps
// streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default: everything beyond serialises).  The runtime reads the variable
// when it initialises, so the library claims its queues here, when it is loaded.  An inherited 4 cannot be told from "nobody
// chose" (launchers export the runtime's default spelled out), and honouring it costs every pipelined entry point a third to two
// thirds of its rate: so a value below the requirement is raised, and a host that limits queues on purpose says so with
// BPGPU_HW_QUEUES (include/bpgpu.h: bpgpu_hw_queues).
#define HW_QUEUES_REQUIRED 24   // 20 ring lanes need 20; beyond ~22 active queues bursts turn erratic
#define HW_QUEUES_MAX 32        // never exported above this
#define HW_QUEUES_UNSET (-1)
#define HW_QUEUES_NOT_A_NUMBER (-2)
// the variable's value as the runtime reads it: the leading decimal integer, whatever follows it
static int hw_queues_parse(const char *s) {
  if (!s) return HW_QUEUES_UNSET;
  char *end = nullptr;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (end == s || errno == ERANGE || v > INT_MAX) return HW_QUEUES_NOT_A_NUMBER;
  return v < 0 ? 0 : (int)v;
}
// The policy, a pure function of the two variables' texts: the number to export, or 0 to leave the process's setting as it is.
//   own (BPGPU_HW_QUEUES), the library's choice as the host states it: "1".."32" exactly that, over whatever was inherited; "0"
//   hands the setting back to the host; anything else is ignored.
//   inherited (GPU_MAX_HW_QUEUES): unset, not a number or below the requirement -> the requirement; at or above it -> untouched
//   (never lowered, and never raised beyond HW_QUEUES_MAX because only the requirement is ever exported here).
static int hw_queues_policy(const char *inherited, const char *own) {
  if (own && *own) {
    char *end = nullptr;
    errno = 0;
    const long v = strtol(own, &end, 10);
    const bool whole = end != own && *end == '\0' && errno != ERANGE && own[0] >= '0' && own[0] <= '9';
    if (whole && v == 0) return 0;
    if (whole && v >= 1 && v <= HW_QUEUES_MAX) return (int)v;
  }
  return hw_queues_parse(inherited) >= HW_QUEUES_REQUIRED ? 0 : HW_QUEUES_REQUIRED;
}
static int g_hw_queues_inherited = HW_QUEUES_UNSET, g_hw_queues_in_force = HW_QUEUES_UNSET;
__attribute__((constructor)) static void bpgpu_claim_hw_queues() {
  const char *inherited = getenv("GPU_MAX_HW_QUEUES");
  g_hw_queues_inherited = hw_queues_parse(inherited);
  const int want = hw_queues_policy(inherited, getenv("BPGPU_HW_QUEUES"));
  if (want > 0) {
    char text[16];
    snprintf(text, sizeof text, "%d", want);
    setenv("GPU_MAX_HW_QUEUES", text, 1);
  }
  g_hw_queues_in_force = hw_queues_parse(getenv("GPU_MAX_HW_QUEUES"));
}
int bpgpu_hw_queues(int *inherited, int *in_force) {
  if (inherited) *inherited = g_hw_queues_inherited;
  if (in_force) *in_force = g_hw_queues_in_force;
  return BPGPU_OK;
}

static int ctx_create(int device, bool single_stream, bpgpu_ctx **out);
static bool horner_group_valid(long long windows) { return windows == 0 || windows == 8 || windows == 16 || windows == 32; }
// the one validator of option values: bpgpu_set_option and the environment seeding of a new context both go through it
static bool opt_valid(int option, int64_t value) {
  if (option <= 0 || option >= BPGPU_OPT_COUNT) return false;
  switch (option) {
    case BPGPU_OPT_MSM_WP_MAX: return value >= 0;                                          // 0 = never
    case BPGPU_OPT_VERIFY_STRAUS_NP: return value >= 1 && value <= 4;
    case BPGPU_OPT_VS_LARGE_MIN: return value >= 1;
    case BPGPU_OPT_TABLE_NP: return value == 0 || value == 1 || value == 2 || value == 4 || value == 8;
    case BPGPU_OPT_IPP_TABLE_MAX_N: return value >= 0;
    case BPGPU_OPT_STREAM_LANES: return value >= 1 && value <= 64;
    case BPGPU_OPT_STREAM_BATCH: return value >= 1 && value <= ((int64_t)1 << 20);
    case BPGPU_OPT_SCREEN_BATCH: return value >= 1 && value <= ((int64_t)1 << 20);
    case BPGPU_OPT_HORNER_FORM: return value >= 0 && value <= 3;
    case BPGPU_OPT_HORNER_ROW_MAX: return value >= 0 && value <= ((int64_t)1 << 20);
    case BPGPU_OPT_PIPPENGER_MIN: return value >= 2 && value <= ((int64_t)1 << 30);
    case BPGPU_OPT_IPP_PIPPENGER_MIN: return value >= 2 && value <= ((int64_t)1 << 30);
    case BPGPU_OPT_FIXED_LPM: return value == 0 || value == 16 || value == 32 || value == 64;
    case BPGPU_OPT_GROUPS_FORM: return value >= 0 && value <= 3;
    case BPGPU_OPT_FIXED_CHUNK_GENS: return value >= -1 && value <= 64;
    case BPGPU_OPT_WITNESS_ROUTE: return value >= 0 && value <= 2;
    case BPGPU_OPT_WITNESS_SCAN_MIN: return value >= 0 && value <= ((int64_t)1 << 25);            // 0 = never
    default: return value == 0 || value == 1;
  }
}
int bpgpu_create(int device, bpgpu_ctx **out) {
  // BPGPU_SINGLE_STREAM=1: one stream per context (deeply pipelined callers overlap ACROSS contexts and
  // hardware queues are a limited resource: GPU_MAX_HW_QUEUES)
  const bool single = getenv("BPGPU_SINGLE_STREAM") && atoi(getenv("BPGPU_SINGLE_STREAM")) != 0;
  return ctx_create(device, single, out);
}
static int ctx_create(int device, bool single, bpgpu_ctx **out) {
  if (!out) return BPGPU_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return BPGPU_E_DEVICE;
  bpgpu_ctx *ctx = new (std::nothrow) bpgpu_ctx();
  if (!ctx) return BPGPU_E_OOM;
  ctx->device = device;
  {
    static const struct { int opt; const char *env; int64_t dflt; } seed[] = {
        {BPGPU_OPT_MSM_WP_MAX, "BPGPU_MSM_WP_MAX", (int64_t)1 << 15}, {BPGPU_OPT_MSM_PIP2_SINGLE, "BPGPU_PIP2_SINGLE", 0},
        {BPGPU_OPT_VERIFY_NO_FUSE, "BPGPU_NO_FUSE", 0},               {BPGPU_OPT_VERIFY_WINDOW_PARALLEL, "BPGPU_WINDOW_PARALLEL", 1},
        {BPGPU_OPT_VERIFY_STRAUS_NP, "BPGPU_STRAUS_NP", 4},           {BPGPU_OPT_IPP_LITERAL, "BPGPU_IPP_LITERAL", 0},
        {BPGPU_OPT_VS_LARGE_MIN, "BPGPU_VS_LARGE_MIN", 4096},         {BPGPU_OPT_TABLE_NP, "BPGPU_TABLE_NP", 0},
        {BPGPU_OPT_IPP_TABLE_MAX_N, "BPGPU_IPP_TABLE_MAX_N", (int64_t)1 << 16},
        {BPGPU_OPT_STREAM_LANES, "BPGPU_STREAM_LANES", 20},           {BPGPU_OPT_STREAM_BATCH, "BPGPU_STREAM_BATCH", 1024},
        {BPGPU_OPT_SCREEN_BATCH, "BPGPU_SCREEN_BATCH", 2560},         {BPGPU_OPT_HORNER_FORM, "BPGPU_HORNER_FORM", 0},
        {BPGPU_OPT_HORNER_ROW_MAX, "BPGPU_HORNER_ROW_MAX", 1536},     {BPGPU_OPT_PIPPENGER_MIN, "BPGPU_PIPPENGER_MIN", 512},
        {BPGPU_OPT_IPP_PIPPENGER_MIN, "BPGPU_IPP_PIPPENGER_MIN", 257}, {BPGPU_OPT_FIXED_LPM, "BPGPU_FIXED_LPM", 0},
        {BPGPU_OPT_GROUPS_FORM, "BPGPU_GROUPS_FORM", 0}, {BPGPU_OPT_FIXED_CHUNK_GENS, "BPGPU_FIXED_CHUNK_GENS", 0},
        {BPGPU_OPT_WITNESS_ROUTE, "BPGPU_WITNESS_ROUTE", 0}, {BPGPU_OPT_WITNESS_SCAN_MIN, "BPGPU_WITNESS_SCAN_MIN", WIT_SCAN_MIN_DEFAULT}};
    // the environment only SEEDS a new context's options, through the same validation as bpgpu_set_option: a value that the
    // setter would refuse (a batch size of 0, a negative lane count, ...) leaves the default in force
    for (auto &s : seed) {
      ctx->opt[s.opt] = s.dflt;
      const char *e = getenv(s.env);
      if (e && *e) {
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end && *end == 0 && opt_valid(s.opt, (int64_t)v)) ctx->opt[s.opt] = (int64_t)v;
      }
    }
    if (const char *e = getenv("BPGPU_HORNER_GROUP"); e && *e) {   // (bpgpu_set_horner_group: seeded the same way)
      char *end = nullptr;
      const long long v = strtoll(e, &end, 10);
      if (end && *end == 0 && horner_group_valid(v)) ctx->horner_group = (int)v;
    }
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking) != hipSuccess ||
      (single ? ((ctx->st2 = ctx->st), hipSuccess) : hipStreamCreateWithFlags(&ctx->st2, hipStreamNonBlocking)) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev1, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev2, hipEventDisableTiming) != hipSuccess ||
      hipMalloc((void **)&ctx->d_flag, sizeof(int)) != hipSuccess) {
    delete ctx;
    return BPGPU_E_DEVICE;
  }
  *out = ctx;
  return BPGPU_OK;
}
void bpgpu_destroy(bpgpu_ctx *ctx) {
  if (!ctx) return;
  for (auto *l : ctx->lanes) bpgpu_destroy(l);
  ctx->lanes.clear();
  if (ctx->lane_ev) hipEventDestroy(ctx->lane_ev);
  if (ctx->pinned) hipHostFree(ctx->pinned);
  if (ctx->wsched_host) hipHostFree(ctx->wsched_host);
  if (ctx->wsched_ev) hipEventDestroy(ctx->wsched_ev);
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->st);
  hipStreamSynchronize(ctx->st2);
  for (auto &s : ctx->ws) if (s.p) hipFree(s.p);
  for (auto &b : ctx->pool) if (b.p) hipFree(b.p);
  hipFree(ctx->d_flag);
  hipFree(ctx->sqrt_tab);
  if (ctx->gen_tab) { hipFree(ctx->gen_tab->points); hipFree(ctx->gen_tab->table); delete ctx->gen_tab; }
  hipEventDestroy(ctx->ev1);
  hipEventDestroy(ctx->ev2);
  for (auto &v : ctx->prof_ev) for (auto e : v) hipEventDestroy(e);
  for (auto e : ctx->prof_pool) hipEventDestroy(e);
  for (auto e : ctx->prof_epochs) hipEventDestroy(e);
  if (ctx->st2 != ctx->st) hipStreamDestroy(ctx->st2);
  hipStreamDestroy(ctx->st);
  delete ctx;
}
const char *bpgpu_last_error(bpgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }
int bpgpu_sync(bpgpu_ctx *ctx) {
  if (!ctx) return BPGPU_E_ARG;
  HIPCK(ctx, hipStreamSynchronize(ctx->st));      // (a stream call joins its lanes into ctx->st before it returns)
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  return BPGPU_OK;
}
void *bpgpu_stream(bpgpu_ctx *ctx) { return ctx ? (void *)ctx->st : nullptr; }
int bpgpu_set_latency_mode(bpgpu_ctx *ctx, int on) {
  if (!ctx) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (on && ctx->st2 == ctx->st) {       // a single-stream context (BPGPU_SINGLE_STREAM): the un-pipelined caller gets its side stream now
    HIPCK(ctx, hipSetDevice(ctx->device));
    hipStream_t s2;
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess) ctx->st2 = s2; else (void)hipGetLastError();
  }
  ctx->latency_mode = on != 0;
  return BPGPU_OK;
}
static void shard_bounds(size_t total, size_t rank, size_t world, size_t *lo, size_t *hi) {   // contiguous, sizes differ by at most one
  const size_t base = total / world, rem = total % world;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}
int bpgpu_set_shard(bpgpu_ctx *ctx, size_t rank, size_t world) {
  if (!ctx || !world || rank >= world) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->shard_rank = rank; ctx->shard_world = world;
  return BPGPU_OK;
}
int bpgpu_set_option(bpgpu_ctx *ctx, int option, int64_t value) {
  if (!ctx || !opt_valid(option, value)) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->opt[option] = value;
  return BPGPU_OK;
}
int bpgpu_set_horner_group(bpgpu_ctx *ctx, int windows) {
  if (!ctx || !horner_group_valid(windows)) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->horner_group = windows;
  return BPGPU_OK;
}
int bpgpu_get_horner_group(bpgpu_ctx *ctx, int *windows) {
  if (!ctx || !windows) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *windows = ctx->horner_group;
  return BPGPU_OK;
}
int bpgpu_get_option(bpgpu_ctx *ctx, int option, int64_t *value) {
  if (!ctx || !value || option <= 0 || option >= BPGPU_OPT_COUNT) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *value = ctx->opt[option];
  return BPGPU_OK;
}
int bpgpu_profile_enable(bpgpu_ctx *ctx, int on) {
  if (!ctx) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->prof = on != 0;
  return BPGPU_OK;
}
int bpgpu_profile_select(bpgpu_ctx *ctx, uint32_t kind_mask) {
  if (!ctx) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (int k = 0; k < BPGPU_PROF_KINDS; k++)      // a pair may not straddle a change of the mask
    if ((ctx->prof_ev[k].size() & 1) || ctx->prof_skip[k]) return BPGPU_E_ARG;
  ctx->prof_mask = kind_mask;
  return BPGPU_OK;
}
int bpgpu_profile_read(bpgpu_ctx *ctx, double ms_sum[BPGPU_PROF_KINDS], uint64_t launches[BPGPU_PROF_KINDS]) {
  if (!ctx || !ms_sum || !launches) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  for (int k = 0; k < BPGPU_PROF_KINDS; k++) { ms_sum[k] = 0; launches[k] = 0; }
  std::vector<bpgpu_ctx *> all{ctx};
  all.insert(all.end(), ctx->lanes.begin(), ctx->lanes.end());     // the lanes of a stream call report through their parent
  for (bpgpu_ctx *c : all) {
    if (c != ctx) HIPCK(ctx, hipStreamSynchronize(c->st));
    for (int k = 0; k < BPGPU_PROF_KINDS; k++) {
      auto &v = c->prof_ev[k];
      for (size_t i = 0; i + 1 < v.size(); i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, v[i], v[i + 1]) == hipSuccess) { ms_sum[k] += ms; launches[k]++; }
      }
      for (auto e : v) c->prof_pool.push_back(e);
      v.clear();
    }
  }
  return BPGPU_OK;
}
// Timed intervals instead of sums: every (start, stop) pair recorded since the last read, in milliseconds relative to `epoch`
// (bpgpu_profile_epoch of ANY context of this device), so that a caller can take the union over kernels, kinds and contexts --
// the time the GPU was busy -- which sums of overlapping launches cannot give.
void *bpgpu_profile_epoch(bpgpu_ctx *ctx) {
  if (!ctx) return nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipEvent_t e = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || hipEventCreate(&e) != hipSuccess) return nullptr;
  if (hipEventRecord(e, ctx->st) != hipSuccess || hipEventSynchronize(e) != hipSuccess) { hipEventDestroy(e); return nullptr; }
  try { ctx->prof_epochs.push_back(e); } catch (const std::bad_alloc &) { hipEventDestroy(e); return nullptr; }
  return (void *)e;                  // owned by the context: valid as a reference until bpgpu_destroy
}
int bpgpu_profile_intervals(bpgpu_ctx *ctx, void *epoch, size_t cap, int32_t *kind, double *start_ms, double *end_ms, size_t *count) {
  if (!ctx || !epoch || !count || (cap && (!kind || !start_ms || !end_ms))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  size_t n = 0;
  std::vector<bpgpu_ctx *> all{ctx};
  all.insert(all.end(), ctx->lanes.begin(), ctx->lanes.end());
  for (bpgpu_ctx *c : all) {
    if (c != ctx) HIPCK(ctx, hipStreamSynchronize(c->st));
    for (int k = 0; k < BPGPU_PROF_KINDS; k++) {
      auto &v = c->prof_ev[k];
      for (size_t i = 0; i + 1 < v.size(); i += 2) {
        float a = 0, b = 0;
        if (n < cap && hipEventElapsedTime(&a, (hipEvent_t)epoch, v[i]) == hipSuccess &&
            hipEventElapsedTime(&b, (hipEvent_t)epoch, v[i + 1]) == hipSuccess) {
          kind[n] = k; start_ms[n] = a; end_ms[n] = b; n++;
        }
      }
      for (auto e : v) c->prof_pool.push_back(e);
      v.clear();
    }
  }
  *count = n;
  return BPGPU_OK;
}
int bpgpu_input_flag(bpgpu_ctx *ctx, int *bad) {
  if (!ctx || !bad) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  CK(flag_read(ctx, bad));
  return flag_reset(ctx);   // read-and-clear: the verification entry points never reset it themselves
}
int bpgpu_host_alloc(size_t bytes, void **out) {
  if (!out) return BPGPU_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return BPGPU_E_DEVICE;
  hipError_t e = hipHostMalloc(out, bytes ? bytes : 4, hipHostMallocDefault);
  if (e != hipSuccess) { *out = nullptr; return e == hipErrorOutOfMemory ? BPGPU_E_OOM : BPGPU_E_DEVICE; }
  return BPGPU_OK;
}
void bpgpu_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}
int bpgpu_malloc(bpgpu_ctx *ctx, size_t bytes, void **dptr) {
  if (!ctx || !dptr) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  HIPCK(ctx, hipMalloc(dptr, bytes ? bytes : 4));
  return BPGPU_OK;
}
int bpgpu_free(bpgpu_ctx *ctx, void *dptr) {
  if (!ctx) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  if (dptr) HIPCK(ctx, hipFree(dptr));
  return BPGPU_OK;
}
int bpgpu_upload(bpgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CK(h2d(ctx, dst, src, bytes));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
// asynchronous on the context's stream: the caller keeps `src` / `dst` alive (and page-locked: bpgpu_host_alloc, for the
// copy to overlap anything) until bpgpu_sync
int bpgpu_upload_async(bpgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return h2d(ctx, dst, src, bytes);
}
int bpgpu_download_async(bpgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return d2h(ctx, dst, src, bytes);
}
int bpgpu_download(bpgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipStreamSynchronize(ctx->st2));
  CK(d2h(ctx, dst, src, bytes));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}

/* ---------------------------------------------------------------- scalar field */
int bpgpu_batch_inverse(bpgpu_ctx *ctx, uint8_t *scalars, size_t n) {
  if (!ctx || (n && !scalars)) return BPGPU_E_ARG;
  if (!n) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *d;
  CK(ws_get(ctx, WS_ARG0, n * 32, &d));
  CK(flag_reset(ctx));
  CK(h2d(ctx, d, scalars, n * 32));
  scalars_check(ctx->st, (Words8 *)d, n, ctx->d_flag);
  batch_inverse(ctx->st, (Words8 *)d, n, ctx->d_flag);
  return checked_download(ctx, {{scalars, d, n * 32}});
}
int bpgpu_inner_product(bpgpu_ctx *ctx, const uint8_t *a, const uint8_t *b, size_t n, uint8_t out[32]) {
  if (!ctx || !out || (n && (!a || !b))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *da, *db, *dout, *scr;
  CK(ws_get(ctx, WS_ARG0, n * 32, &da));
  CK(ws_get(ctx, WS_ARG1, n * 32, &db));
  CK(ws_get(ctx, WS_ARG2, 32, &dout));
  CK(ws_get(ctx, WS_ARG3, inner_product_scratch_bytes(n), &scr));
  CK(flag_reset(ctx));
  CK(h2d(ctx, da, a, n * 32));
  CK(h2d(ctx, db, b, n * 32));
  scalars_check(ctx->st, (Words8 *)da, n, ctx->d_flag);
  scalars_check(ctx->st, (Words8 *)db, n, ctx->d_flag);
  inner_product(ctx->st, (Words8 *)da, (Words8 *)db, n, (Words8 *)dout, scr);
  return checked_download(ctx, {{out, dout, 32}});
}

// MSMs of up to 2^15 terms as a batch of independent <= 32-point sums through the window-parallel launches of the verifier
// (k_ec.hip: point tables -> 64 window sums per group, lane = window -> Horner on quads) and one final sum per instance: no
// sort, no buckets, and the only long dependency chain is the 252 quad doublings every MSM ends in.  64 windows x 16 points is
// 2.4x the additions of the bucket method at these sizes, but they are a few 10^7 wave-instructions on an otherwise idle
// chip: one call is 0.6-0.7 ms from 2 to 2^14 terms and 0.77 ms at 2^15 (the bucket launches of k_pip.hip: 0.86 ms there, and
// ahead from 2^16 terms on: 0.96 against 1.05 ms, 1.07 against 1.59 ms at 2^17; a Straus lane per term + a sum: 1.05 ms).
// points: ABI bytes (validated in the table launch; *d_flag on a malformed one) or, converted = true, AffDev rows.
// *done: handled here (n <= 2^15, BPGPU_OPT_MSM_WP_MAX overrides, and at most 2^16 groups in all).
static void wp_options(const bpgpu_ctx *ctx, VerifyWp &v) {   // the per-context launch-route options of the window-parallel chain
  v.horner_form = (int)ctx->opt[BPGPU_OPT_HORNER_FORM];
  v.row_max = (size_t)ctx->opt[BPGPU_OPT_HORNER_ROW_MAX];
  v.fixed_lpm = (int)ctx->opt[BPGPU_OPT_FIXED_LPM];
  v.groups_form = (int)ctx->opt[BPGPU_OPT_GROUPS_FORM];
  v.fixed_chunk_gens = (int)ctx->opt[BPGPU_OPT_FIXED_CHUNK_GENS];
  v.horner_group = ctx->horner_group;
}
static int msm_wp_batch(bpgpu_ctx *ctx, size_t nb, size_t n, const void *dsc, const void *points, bool converted, JacRaw *dsum, bool *done,
                        int *bad = nullptr, size_t max_n = 0) {
  const size_t wp_max = max_n ? max_n : (size_t)ctx->opt[BPGPU_OPT_MSM_WP_MAX];
  *done = false;
  if (!nb || !n || n > wp_max) return BPGPU_OK;
  size_t G, per;
  if (n <= 32) { G = n; per = 1; }
  else { G = 16; per = (n + 15) / 16; }
  const size_t ng = nb * per, np = per * G;
  if (ng > ((size_t)1 << 16)) return BPGPU_OK;
  const void *sc = dsc, *pts = points;
  if (np != n) {   // ragged tails: identity points with zero scalars -- 64 zero bytes are the identity in either form
    void *dp, *ds;
    CK(ws_get(ctx, WS_WP_PTS, nb * np * 64, &dp));
    CK(ws_get(ctx, WS_WP_SC, nb * np * 32, &ds));
    HIPCK(ctx, hipMemsetAsync(dp, 0, nb * np * 64, ctx->st));
    HIPCK(ctx, hipMemsetAsync(ds, 0, nb * np * 32, ctx->st));
    HIPCK(ctx, hipMemcpy2DAsync(dp, np * 64, points, n * 64, n * 64, nb, hipMemcpyDeviceToDevice, ctx->st));
    HIPCK(ctx, hipMemcpy2DAsync(ds, np * 32, dsc, n * 32, n * 32, nb, hipMemcpyDeviceToDevice, ctx->st));
    pts = dp; sc = ds;
  }
  void *dwp;
  CK(ws_get(ctx, WS_MSM, verify_wp_scratch_bytes(ng, G), &dwp));
  VerifyWp v{(const AffDev *)pts, ng, G, dwp, bad ? bad : ctx->d_flag, nullptr, true, converted};
  wp_options(ctx, v);
  if (!verify_wp_layout_fits(v)) { ctx->err = "internal: window-parallel scratch layout exceeds its buffer (msm)"; return BPGPU_E_DEVICE; }
  VerifyDims d{};
  verify_wp_front_launch(ctx->st, v, d, nullptr, nullptr, 0, false);
  verify_wp_windows(ctx->st, v, (const uint32_t *)sc);
  if (per == 1) {
    verify_wp_groups(ctx->st, v);
    verify_wp_back(ctx->st, v, 8, nullptr, 0, 0, nullptr, 0, nullptr);
    HIPCK(ctx, hipMemcpyAsync(dsum, verify_wp_varsum(v), nb * sizeof(JacRaw), hipMemcpyDeviceToDevice, ctx->st));
  } else {
    // the instances' window sums are added up first: ONE pair of Horner stages per MSM (not per instance, with a sum of `per` points behind it)
    void *dwp2;
    CK(ws_get(ctx, WS_WP_RED, verify_wp_scratch_bytes(nb, G), &dwp2));
    VerifyWp v2 = v;
    v2.nb = nb;
    v2.scratch = dwp2;
    if (!verify_wp_layout_fits(v2)) { ctx->err = "internal: window-parallel scratch layout exceeds its buffer (msm, reduced)"; return BPGPU_E_DEVICE; }
    verify_wp_reduce_instances(ctx->st, v, v2, per);
    verify_wp_groups(ctx->st, v2);
    verify_wp_back(ctx->st, v2, 8, nullptr, 0, 0, nullptr, 0, nullptr);
    HIPCK(ctx, hipMemcpyAsync(dsum, verify_wp_varsum(v2), nb * sizeof(JacRaw), hipMemcpyDeviceToDevice, ctx->st));
  }
  *done = true;
  return BPGPU_OK;
}
/* ---------------------------------------------------------------- MSM (general points) */
// 32-bit bucket ids, sorted entries (term index | sign bit) and offsets: what the bucket method cannot address is BPGPU_E_LEN
static bool pippenger_addressable(size_t nb, size_t n) {
  const int c = pippenger_window(n);
  const size_t cW = 252 / (size_t)c + 1, chalf = (size_t)1 << (c - 1);
  return n < ((size_t)1 << 31) / nb && nb * cW * chalf < ((size_t)1 << 31) && nb * n * cW < ((size_t)1 << 32);
}
int bpgpu_pippenger_plan(size_t nb, size_t n, int32_t out[BPGPU_PIP_PLAN_FIELDS]) {
  if (!out || !nb || n < 2) return BPGPU_E_ARG;
  if (!pippenger_addressable(nb, n)) return BPGPU_E_LEN;
  const PipPlan q = pippenger_plan(nb, n, pippenger_window(n));
  out[BPGPU_PIP_PLAN_C] = q.c;
  out[BPGPU_PIP_PLAN_W] = q.W;
  out[BPGPU_PIP_PLAN_TWO_LEVEL] = q.two_level;
  out[BPGPU_PIP_PLAN_TASK] = (int32_t)q.task;
  out[BPGPU_PIP_PLAN_TASK_SEARCH] = q.task_search;
  out[BPGPU_PIP_PLAN_TASK_SORT] = q.sort_tasks;
  out[BPGPU_PIP_PLAN_SCAN] = q.scan_launches;
  out[BPGPU_PIP_PLAN_COARSE_SCAN] = q.coarse_scan_launches;
  out[BPGPU_PIP_PLAN_FINAL_QUAD] = q.final_quad;
  out[BPGPU_PIP_PLAN_CHUNKS] = q.window_chunks;
  return BPGPU_OK;
}
// one Straus lane per term of dense instances: term i reads pts[i], sc[i]
static StrausArgs straus_dense(const AffDev *pts, const uint32_t *sc) {
  StrausArgs a{};
  a.pts[0] = pts; a.pt_stride[0] = 1;
  a.sc[0] = sc; a.sc_stride[0] = 8;
  return a;
}
// The common end of the variable-base routes, nb validated instances of n terms -> dsum[nb].  From pip_min terms on: the bucket method,
// one batched launch chain over dense instances (pts, sc: nb x n; pippenger() is the same chain for one instance).  Below: one Straus
// lane per term, addressed by `lanes` (results in dres, nb x n), and a tree sum per instance.  Takes WS_PIP or WS_STRAUS.
static int msm_tail(bpgpu_ctx *ctx, size_t nb, size_t n, size_t pip_min, const AffDev *pts, const uint32_t *sc, const StrausArgs &lanes,
                    JacRaw *dres, JacRaw *dsum) {
  if (n >= pip_min) {
    const int c = pippenger_window(n);
    void *dpip;
    CK(ws_get(ctx, WS_PIP, pippenger_scratch_bytes_batch(nb, n, c), &dpip));
    pippenger_batch(ctx->st, pts, sc, nb, n, c, dsum, 1, dpip);
  } else {
    void *dstr;
    CK(straus_ws(ctx, 1, nb * n, &dstr));
    straus(ctx->st, 1, lanes, dres, nb * n, dstr);
    segmented_sum(ctx->st, dres, dsum, nb, n);
  }
  return BPGPU_OK;
}
// device-resident core: dsc / dxy hold the boundary encodings in HBM, dout receives nb x 64 B; asynchronous on ctx->st
static int msm_batch_dev_locked(bpgpu_ctx *ctx, size_t nb, size_t n, const void *dsc, const void *dxy, void *dout) {
  size_t tot = nb * n;
  void *dpts, *dres, *dsum;
  CK(ws_get(ctx, WS_ARG2, tot * sizeof(AffDev), &dpts));
  CK(ws_get(ctx, WS_ARG3, tot * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG4, nb * sizeof(JacRaw), &dsum));
  const size_t pip_min = (size_t)ctx->opt[BPGPU_OPT_PIPPENGER_MIN];
  if (n >= pip_min && !pippenger_addressable(nb, n)) return BPGPU_E_LEN;
  {
    bool done = false;
    scalars_check(ctx->st, (const Words8 *)dsc, tot, ctx->d_flag);
    CK(msm_wp_batch(ctx, nb, n, dsc, dxy, false, (JacRaw *)dsum, &done));
    if (done) {
      jac_to_boundary(ctx->st, (JacRaw *)dsum, (Words8 *)dout, nb);
      return launch_ok(ctx);
    }
  }
  // k_pip2.hip's one-instance pipeline carries the combined batch check; for a lone MSM the window-parallel launches (up to 2^15
  // terms) and k_pip.hip (from 2^16) are both faster now.  BPGPU_OPT_MSM_PIP2_SINGLE routes 2^8..2^16 terms through it (tests).
  const bool pip2_single = ctx->opt[BPGPU_OPT_MSM_PIP2_SINGLE] != 0;
  if (pip2_single && nb == 1 && n >= pip_min && pippenger2_supported(n)) {   // one mid-size instance: seven launches (k_pip2.hip)
    const int c2 = pippenger2_window(n);
    void *dpip;
    CK(ws_get(ctx, WS_PIP, pippenger2_scratch_bytes(n, c2), &dpip));
    pippenger2_boundary(ctx->st, (const Words8 *)dxy, (const Words8 *)dsc, n, c2, (Words8 *)dout, (AffDev *)dpts, dpip, ctx->d_flag);
    return launch_ok(ctx);
  }
  scalars_check(ctx->st, (const Words8 *)dsc, tot, ctx->d_flag);
  points_from_boundary(ctx->st, (const Words8 *)dxy, (AffDev *)dpts, tot, ctx->d_flag);
  CK(msm_tail(ctx, nb, n, pip_min, (const AffDev *)dpts, (const uint32_t *)dsc, straus_dense((const AffDev *)dpts, (const uint32_t *)dsc),
              (JacRaw *)dres, (JacRaw *)dsum));
  jac_to_boundary(ctx->st, (JacRaw *)dsum, (Words8 *)dout, nb);
  return launch_ok(ctx);
}
static int msm_batch_locked(bpgpu_ctx *ctx, size_t nb, size_t n, const uint8_t *scalars, const uint8_t *points,
                            uint8_t *out) {
  HIPCK(ctx, hipSetDevice(ctx->device));
  size_t tot = nb * n;
  if (!nb) return BPGPU_OK;
  if (!n) { memset(out, 0, nb * 64); return BPGPU_OK; }
  void *dsc, *dxy, *dout;
  CK(ws_get(ctx, WS_ARG0, tot * 32, &dsc));
  CK(ws_get(ctx, WS_ARG1, tot * 64, &dxy));
  CK(ws_get(ctx, WS_ARG5, nb * 64, &dout));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dsc, scalars, tot * 32));
  CK(h2d(ctx, dxy, points, tot * 64));
  CK(msm_batch_dev_locked(ctx, nb, n, dsc, dxy, dout));
  return checked_download(ctx, {{out, dout, nb * 64}});
}
int bpgpu_msm_batch_dev(bpgpu_ctx *ctx, size_t nb, size_t n, const void *scalars_dev, const void *points_dev, void *out_dev) {
  if (!ctx || (nb && !out_dev) || (nb && n && (!scalars_dev || !points_dev))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (!nb) return BPGPU_OK;
  if (!n) { HIPCK(ctx, hipMemsetAsync(out_dev, 0, nb * 64, ctx->st)); return BPGPU_OK; }
  CK(flag_reset(ctx));   // the flag reports on the most recent *_dev call
  return msm_batch_dev_locked(ctx, nb, n, scalars_dev, points_dev, out_dev);
}
int bpgpu_msm(bpgpu_ctx *ctx, const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && (!scalars || !points))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return msm_batch_locked(ctx, 1, n, scalars, points, out);
}
int bpgpu_msm_batch(bpgpu_ctx *ctx, size_t nb, size_t n, const uint8_t *scalars, const uint8_t *points,
                    uint8_t *out) {
  if (!ctx || (nb && !out) || (nb && n && (!scalars || !points))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return msm_batch_locked(ctx, nb, n, scalars, points, out);
}

/* ---------------------------------------------------------------- arkworks in-memory forms (k_ark.hip) */
// nb dense instances of sum_i scalars[i] * pts[i] for validated device operands (plain canonical scalars, Montgomery affine points,
// instance-major) -> nb JacRaw
static int msm_core_locked(bpgpu_ctx *ctx, size_t nb, size_t n, const uint32_t *dsc, const AffDev *dpts, JacRaw *dsum) {
  const size_t pip_min = (size_t)ctx->opt[BPGPU_OPT_PIPPENGER_MIN];
  bool done = false;
  CK(msm_wp_batch(ctx, nb, n, dsc, dpts, true, dsum, &done));
  if (done) return BPGPU_OK;
  const bool pip2_single = ctx->opt[BPGPU_OPT_MSM_PIP2_SINGLE] != 0;
  if (pip2_single && nb == 1 && n >= pip_min && pippenger2_supported(n)) {
    const int c2 = pippenger2_window(n);
    void *dpip;
    CK(ws_get(ctx, WS_PIP, pippenger2_scratch_bytes(n, c2), &dpip));
    pippenger2(ctx->st, dpts, dsc, n, c2, dsum, dpip, ctx->d_flag);
    return BPGPU_OK;
  }
  if (n >= pip_min && !pippenger_addressable(nb, n)) return BPGPU_E_LEN;
  void *dres = nullptr;   // the Straus lanes' results: WS_MSM (the caller holds WS_ARG0..5)
  if (n < pip_min) CK(ws_get(ctx, WS_MSM, nb * n * sizeof(JacRaw), &dres));
  return msm_tail(ctx, nb, n, pip_min, dpts, dsc, straus_dense(dpts, dsc), (JacRaw *)dres, dsum);
}
int bpgpu_msm_ark(bpgpu_ctx *ctx, const uint8_t *scalars_mont, const uint8_t *points_jac_mont, size_t n, uint8_t out_jac_mont[96]) {
  if (!ctx || !out_jac_mont || (n && (!scalars_mont || !points_jac_mont))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *dsc, *dpj, *daff, *djac, *dsum, *dout;
  CK(ws_get(ctx, WS_ARG0, (n ? n : 1) * 32, &dsc));
  CK(ws_get(ctx, WS_ARG1, (n ? n : 1) * 96, &dpj));
  CK(ws_get(ctx, WS_ARG2, (n ? n : 1) * sizeof(AffDev), &daff));
  CK(ws_get(ctx, WS_ARG3, (n ? n : 1) * sizeof(JacRaw), &djac));
  CK(ws_get(ctx, WS_ARG4, sizeof(JacRaw), &dsum));
  CK(ws_get(ctx, WS_ARG5, 96, &dout));
  CK(flag_reset(ctx));
  if (n) {
    CK(h2d(ctx, dsc, scalars_mont, n * 32));
    CK(h2d(ctx, dpj, points_jac_mont, n * 96));
    scalars_from_ark(ctx->st, (const Words8 *)dsc, (Words8 *)dsc, n, ctx->d_flag);                 // in place
    points_from_ark(ctx->st, (const Words8 *)dpj, (JacRaw *)djac, n, ctx->d_flag);
    batch_normalize(ctx->st, (const JacRaw *)djac, (AffDev *)daff, n, 8);
    CK(msm_core_locked(ctx, 1, n, (const uint32_t *)dsc, (const AffDev *)daff, (JacRaw *)dsum));
  } else {
    HIPCK(ctx, hipMemsetAsync(dsum, 0, sizeof(JacRaw), ctx->st));                                  // Z = 0: the identity
  }
  points_to_ark(ctx->st, (const JacRaw *)dsum, (Words8 *)dout, 1);
  return checked_download(ctx, {{out_jac_mont, dout, 96}});
}
static int ark_convert_locked(bpgpu_ctx *ctx, int what, const uint8_t *in, size_t n, uint8_t *out) {
  static const size_t in_sz[4] = {32, 32, 96, 64}, out_sz[4] = {32, 32, 64, 96};
  if (!n) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *din, *dout, *djac, *daff;
  CK(ws_get(ctx, WS_ARG0, n * in_sz[what], &din));
  CK(ws_get(ctx, WS_ARG1, n * out_sz[what], &dout));
  CK(ws_get(ctx, WS_ARG3, n * sizeof(JacRaw), &djac));
  CK(ws_get(ctx, WS_ARG2, n * sizeof(AffDev), &daff));
  CK(flag_reset(ctx));
  CK(h2d(ctx, din, in, n * in_sz[what]));
  switch (what) {
    case 0: scalars_from_ark(ctx->st, (const Words8 *)din, (Words8 *)dout, n, ctx->d_flag); break;
    case 1: scalars_to_ark(ctx->st, (const Words8 *)din, (Words8 *)dout, n, ctx->d_flag); break;
    case 2:
      points_from_ark(ctx->st, (const Words8 *)din, (JacRaw *)djac, n, ctx->d_flag);
      jac_to_boundary(ctx->st, (const JacRaw *)djac, (Words8 *)dout, n);
      break;
    default:
      points_from_boundary(ctx->st, (const Words8 *)din, (AffDev *)daff, n, ctx->d_flag);
      aff_to_jacraw(ctx->st, (const AffDev *)daff, (JacRaw *)djac, n);
      points_to_ark(ctx->st, (const JacRaw *)djac, (Words8 *)dout, n);
      break;
  }
  return checked_download(ctx, {{out, dout, n * out_sz[what]}});
}
int bpgpu_scalars_from_ark(bpgpu_ctx *ctx, const uint8_t *scalars_mont, size_t n, uint8_t *scalars_le) {
  if (!ctx || (n && (!scalars_mont || !scalars_le))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ark_convert_locked(ctx, 0, scalars_mont, n, scalars_le);
}
int bpgpu_scalars_to_ark(bpgpu_ctx *ctx, const uint8_t *scalars_le, size_t n, uint8_t *scalars_mont) {
  if (!ctx || (n && (!scalars_mont || !scalars_le))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ark_convert_locked(ctx, 1, scalars_le, n, scalars_mont);
}
int bpgpu_points_from_ark(bpgpu_ctx *ctx, const uint8_t *points_jac_mont, size_t n, uint8_t *points_xy) {
  if (!ctx || (n && (!points_jac_mont || !points_xy))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ark_convert_locked(ctx, 2, points_jac_mont, n, points_xy);
}
int bpgpu_points_to_ark(bpgpu_ctx *ctx, const uint8_t *points_xy, size_t n, uint8_t *points_jac_mont) {
  if (!ctx || (n && (!points_jac_mont || !points_xy))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ark_convert_locked(ctx, 3, points_xy, n, points_jac_mont);
}
int bpgpu_points_sum(bpgpu_ctx *ctx, const uint8_t *points, size_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && !points)) return BPGPU_E_ARG;
  if (!n) { memset(out, 0, 64); return BPGPU_OK; }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *dxy, *dout;
  CK(ws_get(ctx, WS_ARG0, n * 64, &dxy));
  CK(ws_get(ctx, WS_ARG4, 64, &dout));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dxy, points, n * 64));
  points_sum(ctx->st, (const Words8 *)dxy, n, (Words8 *)dout, ctx->d_flag);
  return checked_download(ctx, {{out, dout, 64}});
}
/* nsets MSMs over ONE point vector (the share / MAC / public-modifier MSMs of msm_authenticated_iter) */
int bpgpu_msm_shared(bpgpu_ctx *ctx, size_t nsets, size_t n, const uint8_t *scalars, const uint8_t *points,
                     uint8_t *out) {
  if (!ctx || (nsets && !out) || (nsets && n && (!scalars || !points))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (!nsets) return BPGPU_OK;
  if (!n) { memset(out, 0, nsets * 64); return BPGPU_OK; }
  const size_t tot = nsets * n;
  void *dsc, *dxy, *dpts, *dres, *dsum, *dout;
  CK(ws_get(ctx, WS_ARG0, tot * 32, &dsc));
  CK(ws_get(ctx, WS_ARG1, n * 64, &dxy));
  CK(ws_get(ctx, WS_ARG3, tot * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG4, nsets * sizeof(JacRaw), &dsum));
  CK(ws_get(ctx, WS_ARG5, nsets * 64, &dout));
  const size_t pip_min = (size_t)ctx->opt[BPGPU_OPT_PIPPENGER_MIN];
  const bool bucket = n >= pip_min;
  CK(ws_get(ctx, WS_ARG2, (bucket ? tot + n : n) * sizeof(AffDev), &dpts));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dsc, scalars, tot * 32));
  CK(h2d(ctx, dxy, points, n * 64));
  scalars_check(ctx->st, (Words8 *)dsc, tot, ctx->d_flag);
  points_from_boundary(ctx->st, (Words8 *)dxy, (AffDev *)dpts, n, ctx->d_flag);   // validated and converted once
  bool wp_done = false;
  if (!bucket || n <= ((size_t)1 << 15)) {   // window-parallel launches over replicas of the converted points (msm_wp_batch)
    void *drep;
    CK(ws_get(ctx, WS_VFIX, tot * sizeof(AffDev), &drep));
    gather_points(ctx->st, (AffDev *)dpts, 0, n, nsets, (AffDev *)drep, n);
    CK(msm_wp_batch(ctx, nsets, n, dsc, drep, true, (JacRaw *)dsum, &wp_done));
  }
  if (!wp_done) {
    // the bucket method's instances read replicas of the converted points; the Straus lanes (set, term) share the one point array
    AffDev *rep = (AffDev *)dpts + n;   // (behind the n converted points; there, and read, only when bucket)
    if (bucket) gather_points(ctx->st, (AffDev *)dpts, 0, n, nsets, rep, n);
    StrausArgs a = straus_dense((const AffDev *)dpts, (const uint32_t *)dsc);
    a.pt_outer[0] = 0; a.sc_outer[0] = n * 8;
    a.inner = n;
    CK(msm_tail(ctx, nsets, n, pip_min, rep, (const uint32_t *)dsc, a, (JacRaw *)dres, (JacRaw *)dsum));
  }
  jac_to_boundary(ctx->st, (JacRaw *)dsum, (Words8 *)dout, nsets);
  return checked_download(ctx, {{out, dout, nsets * 64}});
}

/* ---------------------------------------------------------------- point wire codec */
int bpgpu_points_decompress(bpgpu_ctx *ctx, const uint8_t *compressed, size_t n, uint8_t *xy, int32_t *ok) {
  if (!ctx || (n && (!compressed || !xy || !ok))) return BPGPU_E_ARG;
  if (!n) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (!ctx->sqrt_tab) {
    void *t = nullptr;
    if (hipMalloc(&t, sqrt_table_bytes()) != hipSuccess) return BPGPU_E_OOM;
    sqrt_tables_build(ctx->st, t);
    ctx->sqrt_tab = t;
  }
  void *din, *dxy, *dok;
  CK(ws_get(ctx, WS_ARG0, n * 32, &din));
  CK(ws_get(ctx, WS_ARG1, n * 64, &dxy));
  CK(ws_get(ctx, WS_ARG5, n * 4, &dok));
  CK(h2d(ctx, din, compressed, n * 32));
  points_decompress(ctx->st, (const Words8 *)din, (Words8 *)dxy, (int32_t *)dok, n, ctx->sqrt_tab);
  CK(launch_ok(ctx));
  CK(d2h(ctx, xy, dxy, n * 64));
  CK(d2h(ctx, ok, dok, n * 4));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
int bpgpu_points_compress(bpgpu_ctx *ctx, const uint8_t *xy, size_t n, uint8_t *compressed) {
  if (!ctx || (n && (!xy || !compressed))) return BPGPU_E_ARG;
  if (!n) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *dxy, *dpts, *dout;
  CK(ws_get(ctx, WS_ARG1, n * 64, &dxy));
  CK(ws_get(ctx, WS_ARG2, n * sizeof(AffDev), &dpts));
  CK(ws_get(ctx, WS_ARG0, n * 32, &dout));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dxy, xy, n * 64));
  points_from_boundary(ctx->st, (const Words8 *)dxy, (AffDev *)dpts, n, ctx->d_flag);   // canonical + on-curve checks
  points_compress(ctx->st, (const Words8 *)dxy, (Words8 *)dout, n);
  return checked_download(ctx, {{compressed, dout, n * 32}});
}

/* ---------------------------------------------------------------- resident generators */
int bpgpu_gens_create(bpgpu_ctx *ctx, const uint8_t *G, const uint8_t *H, size_t cap, const uint8_t B[64],
                      const uint8_t Bb[64], int c, bpgpu_gens **out) try {
  if (!ctx || !out || !B || !Bb || (cap && (!G || !H))) return BPGPU_E_ARG;
  if (!(c == 4 || c == 8 || c == 10 || c == 12 || c == 14 || c == 16 || c == 20)) return BPGPU_E_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  size_t ng = 2 + 2 * cap;
  std::vector<uint8_t> host(ng * 64);   // (before `g`: a bad_alloc here must not leak it)
  bpgpu_gens *g = new (std::nothrow) bpgpu_gens();
  if (!g) return BPGPU_E_OOM;
  g->cap = cap;
  g->c = c;
  memcpy(&host[0], B, 64);
  memcpy(&host[64], Bb, 64);
  if (cap) { memcpy(&host[128], G, cap * 64); memcpy(&host[128 + cap * 64], H, cap * 64); }
  size_t entries = fixed_table_entries(c, ng);
  size_t W = 252 / c + 1;
  void *dxy = nullptr, *scratch = nullptr;
  auto fail = [&](int rc) {
    if (dxy) hipFree(dxy);
    if (scratch) hipFree(scratch);
    if (g->points) hipFree(g->points);
    if (g->table) hipFree(g->table);
    delete g;
    return rc;
  };
#define GCK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e__); return fail(e__ == hipErrorOutOfMemory ? BPGPU_E_OOM : BPGPU_E_DEVICE); } } while (0)
  GCK(hipMalloc(&dxy, ng * 64));
  GCK(hipMalloc((void **)&g->points, ng * sizeof(AffDev)));
  GCK(hipMalloc((void **)&g->table, entries * sizeof(AffDev)));
  // the Jacobian staging of the table is built for groups of generators so that it stays below ~8 GB
  // (a 20-bit-window table of the 64-bit gadget's 130 generators is 57 GB; staged whole it would need 95 GB more)
  const size_t per_gen = W * ((size_t)1 << (c - 1));                 // table rows per generator
  size_t group = ((size_t)8 << 30) / ((per_gen + W) * sizeof(JacRaw));
  if (group < 1) group = 1;
  if (group > ng) group = ng;
  GCK(hipMalloc(&scratch, group * (W + per_gen) * sizeof(JacRaw)));
  GCK(hipMemsetAsync(ctx->d_flag, 0, sizeof(int), ctx->st));
  GCK(hipMemcpyAsync(dxy, host.data(), ng * 64, hipMemcpyHostToDevice, ctx->st));
  points_from_boundary(ctx->st, (Words8 *)dxy, g->points, ng, ctx->d_flag);
  for (size_t g0 = 0; g0 < ng; g0 += group) {
    size_t cnt = ng - g0 < group ? ng - g0 : group;
    fixed_table_build(ctx->st, c, g->points + g0, cnt, g->table + g0 * per_gen, (JacRaw *)scratch);
  }
  GCK(hipGetLastError());
  int bad = 0;
  GCK(hipMemcpyAsync(&bad, ctx->d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
  GCK(hipStreamSynchronize(ctx->st));
#undef GCK
  hipFree(dxy); dxy = nullptr;
  hipFree(scratch); scratch = nullptr;
  if (bad) return fail(BPGPU_E_ARG);
  *out = g;
  return BPGPU_OK;
} catch (const std::bad_alloc &) {   // host-side staging (std::vector): no exception crosses the C ABI
  return BPGPU_E_OOM;
}
void bpgpu_gens_destroy(bpgpu_ctx *ctx, bpgpu_gens *g) {
  if (!g) return;
  if (ctx) { std::lock_guard<std::mutex> lk(ctx->mu); hipStreamSynchronize(ctx->st); hipStreamSynchronize(ctx->st2); }
  hipFree(g->points);
  hipFree(g->table);
  delete g;
}
size_t bpgpu_gens_capacity(const bpgpu_gens *g) { return g ? g->cap : 0; }

// ark = the scalars are ark-ff Montgomery limbs (x 2^256 mod n, what the reference's Scalar holds in memory): converted in
// place on the device (one multiplication per scalar) instead of one de-Montgomery per scalar on the host
static int msm_gens_impl(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *scalars, uint8_t *out, bool ark) {
  if (!ctx || !g || (nb && (!scalars || !out))) return BPGPU_E_ARG;
  if (n > g->cap) return BPGPU_E_GENS;
  if (!nb) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  size_t per = 2 + 2 * n, tot = nb * per;
  void *dsc, *dres, *dout;
  CK(ws_get(ctx, WS_ARG0, tot * 32, &dsc));
  CK(ws_get(ctx, WS_ARG4, nb * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG5, nb * 64, &dout));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dsc, scalars, tot * 32));
  ProfSpan span(ctx, 18, ctx->st);
  if (ark) scalars_from_ark(ctx->st, (const Words8 *)dsc, (Words8 *)dsc, tot, ctx->d_flag);
  else scalars_check(ctx->st, (Words8 *)dsc, tot, ctx->d_flag);
  CK(msm_gens_dev(ctx, g, nb, n, (uint32_t *)dsc, (JacRaw *)dres, ctx->st));
  jac_to_boundary(ctx->st, (JacRaw *)dres, (Words8 *)dout, nb);
  span.close();
  return checked_download(ctx, {{out, dout, nb * 64}});
}
int bpgpu_msm_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *scalars, uint8_t *out) {
  return msm_gens_impl(ctx, g, nb, n, scalars, out, false);
}
int bpgpu_msm_gens_ark(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *scalars_ark, uint8_t *out) {
  return msm_gens_impl(ctx, g, nb, n, scalars_ark, out, true);
}

/* ---------------------------------------------------------------- IPP */
int bpgpu_fold_witness(bpgpu_ctx *ctx, size_t n, const uint8_t u[32], const uint8_t u_inv[32], const uint8_t *a,
                       const uint8_t *b, const uint8_t *G, const uint8_t *H, uint8_t *a_out, uint8_t *b_out,
                       uint8_t *G_out, uint8_t *H_out) {
  if (!ctx || !u || !u_inv || (n && (!a || !b || !G || !H || !a_out || !b_out || !G_out || !H_out))) return BPGPU_E_ARG;
  if (!n) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  // scalars: u, u_inv, a[2n], b[2n], a_out[n], b_out[n]
  void *dsc, *dxy, *dpts, *dres, *dout;
  size_t nsc = 2 + 4 * n + 2 * n;
  CK(ws_get(ctx, WS_ARG0, nsc * 32, &dsc));
  CK(ws_get(ctx, WS_ARG1, 4 * n * 64, &dxy));
  CK(ws_get(ctx, WS_ARG2, 4 * n * sizeof(AffDev), &dpts));
  CK(ws_get(ctx, WS_ARG3, 2 * n * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG5, 2 * n * 64, &dout));
  Words8 *w = (Words8 *)dsc;
  Words8 *du = w, *dui = w + 1, *da = w + 2, *db = w + 2 + 2 * n, *dao = w + 2 + 4 * n, *dbo = w + 2 + 5 * n;
  CK(flag_reset(ctx));
  CK(h2d(ctx, du, u, 32));
  CK(h2d(ctx, dui, u_inv, 32));
  CK(h2d(ctx, da, a, 2 * n * 32));
  CK(h2d(ctx, db, b, 2 * n * 32));
  CK(h2d(ctx, dxy, G, 2 * n * 64));
  CK(h2d(ctx, (uint8_t *)dxy + 2 * n * 64, H, 2 * n * 64));
  scalars_check(ctx->st, w, 2 + 4 * n, ctx->d_flag);
  points_from_boundary(ctx->st, (Words8 *)dxy, (AffDev *)dpts, 4 * n, ctx->d_flag);
  fold_scalars(ctx->st, n, du, dui, da, db, dao, dbo);
  AffDev *dG = (AffDev *)dpts, *dH = dG + 2 * n;
  StrausArgs sg{};   // G' = u^-1 G_L + u G_R
  sg.pts[0] = dG; sg.pts[1] = dG + n; sg.pt_stride[0] = sg.pt_stride[1] = 1;
  sg.sc[0] = (uint32_t *)dui; sg.sc[1] = (uint32_t *)du; sg.sc_stride[0] = sg.sc_stride[1] = 0;
  void *dstr;
  CK(straus_ws(ctx, 2, n, &dstr));
  straus(ctx->st, 2, sg, (JacRaw *)dres, n, dstr);
  StrausArgs sh{};   // H' = u H_L + u^-1 H_R
  sh.pts[0] = dH; sh.pts[1] = dH + n; sh.pt_stride[0] = sh.pt_stride[1] = 1;
  sh.sc[0] = (uint32_t *)du; sh.sc[1] = (uint32_t *)dui; sh.sc_stride[0] = sh.sc_stride[1] = 0;
  straus(ctx->st, 2, sh, (JacRaw *)dres + n, n, dstr);
  jac_to_boundary(ctx->st, (JacRaw *)dres, (Words8 *)dout, 2 * n);
  return checked_download(ctx, {{a_out, dao, n * 32}, {b_out, dbo, n * 32}, {G_out, dout, n * 64}, {H_out, (uint8_t *)dout + n * 64, n * 64}});
}
int bpgpu_verification_scalars(bpgpu_ctx *ctx, const uint8_t *challenges, size_t k, size_t n, uint8_t *u_sq,
                               uint8_t *u_inv_sq, uint8_t *s) {
  if (!ctx || !s || (k && (!challenges || !u_sq || !u_inv_sq))) return BPGPU_E_ARG;
  if (k >= 32 || n != ((size_t)1 << k)) return BPGPU_E_LEN;   // inner_product_proof.rs:259-267
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *d;
  CK(ws_get(ctx, WS_ARG0, (3 * k + n + 1) * 32, &d));
  Words8 *w = (Words8 *)d;
  CK(flag_reset(ctx));
  CK(h2d(ctx, w, challenges, k * 32));
  scalars_check(ctx->st, w, k, ctx->d_flag);
  verification_scalars(ctx->st, w, k, n, w + k, w + 2 * k, w + 3 * k);
  return checked_download(ctx, {{u_sq, w + k, k * 32}, {u_inv_sq, w + 2 * k, k * 32}, {s, w + 3 * k, n * 32}});
}

/* ---------------------------------------------------------------- InnerProductProof::verify (k_ippv.hip) */
namespace {
struct IppvOps {   // device pointers; Qw: Q (nb points) or, over resident generators, w (nb scalars); ch: challenges or, fs, states_in
  const void *Qw, *Gf, *Hf, *G, *H, *P, *L, *R, *ab, *ch;
};
}
static int ippv_dims(size_t n, size_t k) { return (k >= 32 || n != ((size_t)1 << k)) ? BPGPU_E_LEN : BPGPU_OK; }   // inner_product_proof.rs:259-267
// the instance length the variable-base routes get: above 32 terms the window-parallel launches take groups of 16, so the
// instances are laid out padded (identity points, zero scalars) instead of being copied into a padded layout by msm_wp_batch
static size_t ippv_stride(size_t terms) { return terms <= 32 ? terms : (terms + 15) / 16 * 16; }
// device operands -> ok (nb int32), expect_P (optional, nb x 64 B), states_out (fs, optional); asynchronous on ctx->st, malformed
// operands raise ctx->d_flag (reset by the caller)
static int ippv_dev_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, bool shared, const IppvOps &in, bool fs,
                           void *ok, void *expect_P, void *states_out) {
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (!ippv_assemble_fits(nb, n)) return BPGPU_E_LEN;
  const size_t terms = g ? 2 * k : 2 * n + 1 + 2 * k, stride = ippv_stride(terms), fixed = 2 + 2 * n;
  void *dhdr, *dsc, *dvsc = nullptr, *dpts, *dsum, *dch = nullptr;
  const size_t hdr_bytes = (nb * (k + 2) * bp::NL * 4 + 63) / 64 * 64;
  CK(ws_get(ctx, WS_IPPV_HDR, hdr_bytes + nb * 4, &dhdr));
  int32_t *dreject = (int32_t *)((uint8_t *)dhdr + hdr_bytes);
  CK(ws_get(ctx, WS_IPPV_SC, nb * (g ? fixed : stride) * 32, &dsc));
  if (g) CK(ws_get(ctx, WS_IPPV_VSC, nb * stride * 32, &dvsc));
  CK(ws_get(ctx, WS_IPPV_PTS, nb * stride * sizeof(AffDev), &dpts));
  CK(ws_get(ctx, WS_IPPV_SUM, nb * (2 * sizeof(JacRaw) + 64 + 4), &dsum));
  JacRaw *dvar = (JacRaw *)dsum, *dfix = dvar + nb;
  Words8 *dexp = expect_P ? (Words8 *)expect_P : (Words8 *)(dfix + nb);
  HIPCK(ctx, hipMemsetAsync(dreject, 0, nb * 4, ctx->st));
  const Words8 *ch = (const Words8 *)in.ch;
  if (fs) {
    CK(ws_get(ctx, WS_FS_CH, nb * (k ? k : 1) * 32, &dch));
    ippv_transcript(ctx->st, nb, k, (const Words8 *)in.ch, (const Words8 *)in.L, (const Words8 *)in.R, (Words8 *)dch, dreject, (Words8 *)states_out);
    ch = (const Words8 *)dch;
  }
  // scalars: [G | H | Q | L | R | padding] per dense instance; over resident generators [B, B_blinding, G.., H..] and [L | R | padding]
  Words8 *sc = (Words8 *)dsc, *vsc = g ? (Words8 *)dvsc : sc + 2 * n + 1;
  IppvHeader h{nb, (int)k, ch, (const Words8 *)in.ab, g ? (const Words8 *)in.Qw : nullptr, (int32_t *)dhdr,
               g ? sc : sc + 2 * n, g ? sc + 1 : nullptr, g ? fixed : stride, vsc, vsc + k, stride, dreject, ctx->d_flag};
  ippv_header(ctx->st, h);
  ippv_assemble(ctx->st, nb, n, k, (const int32_t *)dhdr, (const Words8 *)in.Gf, (const Words8 *)in.Hf, g ? sc + 2 : sc, g ? sc + 2 + n : sc + n,
                g ? fixed : stride, ctx->d_flag);
  IppvPoints pa{};
  int ns = 0;
  if (!g) {
    pa.seg[ns++] = {(const Words8 *)in.G, shared ? 0 : n, n, 0};
    pa.seg[ns++] = {(const Words8 *)in.H, shared ? 0 : n, n, 0};
    pa.seg[ns++] = {(const Words8 *)in.Qw, 1, 1, 0};
  }
  pa.seg[ns++] = {(const Words8 *)in.L, k, k, 0};
  pa.seg[ns++] = {(const Words8 *)in.R, k, k, 0};
  pa.seg[ns++] = {(const Words8 *)in.P, 1, 1, 1};
  pa.nseg = ns; pa.nb = nb; pa.stride = stride; pa.used = terms; pa.extra = 1;
  pa.dst = (AffDev *)dpts; pa.pad_sc = g ? (Words8 *)dvsc : sc; pa.bad = ctx->d_flag;
  ippv_points(ctx->st, pa);
  if (stride) CK(msm_core_locked(ctx, nb, stride, (const uint32_t *)(g ? dvsc : dsc), (const AffDev *)dpts, dvar));
  if (g) {
    CK(msm_gens_dev(ctx, g, nb, n, (const uint32_t *)dsc, dfix, ctx->st, WS_MSM2));
    verify_finalize(ctx->st, dvar, stride ? 1 : 0, dfix, nb, (int32_t *)ok, dexp);   // ok: overwritten by the verdict below
  } else {
    jac_to_boundary(ctx->st, dvar, dexp, nb);
  }
  ippv_verdict(ctx->st, nb, dexp, (const Words8 *)in.P, dreject, (int32_t *)ok);
  return launch_ok(ctx);
}
// the host-pointer forms after their argument checks: the operands go up in one staging buffer, verdicts (and expect_P /
// states_out) come back; a malformed operand is BPGPU_E_ARG
static int ippv_host(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, bool shared, const IppvOps &in, bool fs, int32_t *ok,
                     uint8_t *expect_P, uint8_t *states_out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t gtot = g ? 0 : (shared ? n : nb * n);
  const size_t sizes[10] = {nb * (g ? 32 : 64), nb * n * 32, nb * n * 32, gtot * 64, gtot * 64, nb * 64, nb * k * 64, nb * k * 64, nb * 64,
                            fs ? nb * 32 : nb * k * 32};
  const void *host[10] = {in.Qw, in.Gf, in.Hf, in.G, in.H, in.P, in.L, in.R, in.ab, in.ch};
  size_t off[11] = {0};
  for (int i = 0; i < 10; i++) off[i + 1] = off[i] + sizes[i];
  const size_t o_ok = off[10], o_exp = (o_ok + nb * 4 + 63) / 64 * 64, o_st = o_exp + nb * 64;
  void *d;
  CK(ws_get(ctx, WS_IPPV_STAGE, o_st + nb * 32, &d));
  uint8_t *b = (uint8_t *)d;
  CK(flag_reset(ctx));
  for (int i = 0; i < 10; i++) CK(h2d(ctx, b + off[i], host[i], sizes[i]));
  const IppvOps dev{b + off[0], b + off[1], b + off[2], b + off[3], b + off[4], b + off[5], b + off[6], b + off[7], b + off[8], b + off[9]};
  CK(ippv_dev_locked(ctx, g, nb, n, k, shared, dev, fs, b + o_ok, expect_P ? b + o_exp : nullptr, fs && states_out ? b + o_st : nullptr));
  return checked_download(ctx, {{ok, b + o_ok, nb * 4}, {expect_P, b + o_exp, expect_P ? nb * 64 : 0},
                                {states_out, b + o_st, fs && states_out ? nb * 32 : 0}});
}
// the operands every form needs (L, R, challenges only from k = 1 on)
static bool ippv_args(const void *Gf, const void *Hf, const void *P, const void *L, const void *R, const void *ab, const void *ch, size_t k,
                      bool fs, const void *ok) {
  return Gf && Hf && P && ab && ok && (fs ? ch != nullptr : (!k || ch)) && (!k || (L && R));
}
int bpgpu_ipp_verify_batch(bpgpu_ctx *ctx, size_t nb, size_t n, size_t k, const uint8_t *Q, const uint8_t *G_factors, const uint8_t *H_factors,
                           const uint8_t *G, const uint8_t *H, int shared_gens, const uint8_t *P, const uint8_t *L, const uint8_t *R,
                           const uint8_t *ab, const uint8_t *challenges, int32_t *ok, uint8_t *expect_P) {
  if (!ctx || (nb && (!Q || !G || !H || !ippv_args(G_factors, H_factors, P, L, R, ab, challenges, k, false, ok)))) return BPGPU_E_ARG;
  CK(ippv_dims(n, k));
  if (!nb) return BPGPU_OK;
  return ippv_host(ctx, nullptr, nb, n, k, shared_gens != 0, {Q, G_factors, H_factors, G, H, P, L, R, ab, challenges}, false, ok, expect_P, nullptr);
}
int bpgpu_ipp_verify_batch_dev(bpgpu_ctx *ctx, size_t nb, size_t n, size_t k, const void *Q, const void *G_factors, const void *H_factors,
                               const void *G, const void *H, int shared_gens, const void *P, const void *L, const void *R, const void *ab,
                               const void *challenges, void *ok, void *expect_P) {
  if (!ctx || (nb && (!Q || !G || !H || !ippv_args(G_factors, H_factors, P, L, R, ab, challenges, k, false, ok)))) return BPGPU_E_ARG;
  CK(ippv_dims(n, k));
  if (!nb) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  CK(flag_reset(ctx));   // the flag reports on the most recent *_dev call
  return ippv_dev_locked(ctx, nullptr, nb, n, k, shared_gens != 0, {Q, G_factors, H_factors, G, H, P, L, R, ab, challenges}, false, ok, expect_P,
                         nullptr);
}
int bpgpu_ipp_verify_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, const uint8_t *w, const uint8_t *G_factors,
                          const uint8_t *H_factors, const uint8_t *P, const uint8_t *L, const uint8_t *R, const uint8_t *ab,
                          const uint8_t *challenges, int32_t *ok, uint8_t *expect_P) {
  if (!ctx || !g || (nb && (!w || !ippv_args(G_factors, H_factors, P, L, R, ab, challenges, k, false, ok)))) return BPGPU_E_ARG;
  CK(ippv_dims(n, k));
  if (n > g->cap) return BPGPU_E_GENS;
  if (!nb) return BPGPU_OK;
  return ippv_host(ctx, g, nb, n, k, true, {w, G_factors, H_factors, nullptr, nullptr, P, L, R, ab, challenges}, false, ok, expect_P, nullptr);
}
int bpgpu_ipp_verify_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, const uint8_t *Q_or_w, const uint8_t *G_factors,
                        const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int shared_gens, const uint8_t *P, const uint8_t *L,
                        const uint8_t *R, const uint8_t *ab, const uint8_t *states_in, int32_t *ok, uint8_t *states_out) {
  if (!ctx || (nb && (!Q_or_w || (!g && (!G || !H)) || !ippv_args(G_factors, H_factors, P, L, R, ab, states_in, k, true, ok)))) return BPGPU_E_ARG;
  CK(ippv_dims(n, k));
  if (g && n > g->cap) return BPGPU_E_GENS;
  if (!nb) return BPGPU_OK;
  return ippv_host(ctx, g, nb, n, k, g || shared_gens != 0, {Q_or_w, G_factors, H_factors, g ? nullptr : G, g ? nullptr : H, P, L, R, ab, states_in},
                   true, ok, nullptr, states_out);
}

/* ---------------------------------------------------------------- R1CS */
static int circuit_create_impl(bpgpu_ctx *ctx, size_t q_real, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                               const uint32_t *idx, const uint8_t *coeff, size_t n_mul, size_t m, bpgpu_circuit **out, bool ark = false) try {
  if (!ctx || !out || !row_ptr) return BPGPU_E_ARG;
  *out = nullptr;
  const size_t q = q_real * (1 + nchi);     // CSR rows: block j (rows j q_real ..) holds the chi_j parts of the coefficients
  size_t nnz = row_ptr[q];
  if (nnz && (!kind || !idx || !coeff)) return BPGPU_E_ARG;
  // CSR (row-major, as the reference holds constraints) -> column-major by output variable, on the device (k_scalar.hip
  // circuit_transpose): the host only checks that the row pointers are monotone.  (The transposition used to run here, single-
  // threaded: 2 ms for the 2^14-shuffle's 196 600 terms, paid by every proof of a circuit with randomized constraints.)
  size_t nout = 3 * n_mul + m + 1;
  for (size_t r = 0; r < q; r++) if (row_ptr[r + 1] < row_ptr[r]) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  bpgpu_circuit *c = new (std::nothrow) bpgpu_circuit();
  if (!c) return BPGPU_E_OOM;
  c->q = q_real; c->n = n_mul; c->m = m; c->nnz = nnz; c->nchi = nchi;
  // (plain allocations, not the context's pool: a circuit is shared by contexts and may outlive the one that made it)
  // ONE allocation [coeff | col_ptr | row] (a proof of a circuit with randomized constraints pays for this every time: three
  // hipMalloc + three hipFree were ~1 ms of the 2^14-shuffle's prove and verify)
  auto fail = [&](int rc) { hipFree(c->coeff); delete c; return rc; };
  const size_t b_coeff = (nnz ? nnz : 1) * 32, b_col = ((nout + 1) * 4 + 255) / 256 * 256, b_row = (nnz ? nnz : 1) * 4;
  if (hipMalloc((void **)&c->coeff, b_coeff + b_col + b_row) != hipSuccess) { c->coeff = nullptr; return fail(BPGPU_E_OOM); }
  c->col_ptr = (uint32_t *)((uint8_t *)c->coeff + b_coeff);
  c->row = (uint32_t *)((uint8_t *)c->coeff + b_coeff + b_col);
  void *drp, *dkd, *dix, *dcf, *dfill;
  int rc;
  if ((rc = ws_get(ctx, WS_ARG0, (q + 1) * 4, &drp)) || (rc = ws_get(ctx, WS_ARG1, (nnz ? nnz : 1) * 4, &dkd)) || (rc = ws_get(ctx, WS_ARG2, (nnz ? nnz : 1) * 4, &dix)) ||
      (rc = ws_get(ctx, WS_ARG3, (nnz ? nnz : 1) * 32, &dcf)) || (rc = ws_get(ctx, WS_ARG4, nout * 4, &dfill)))
    return fail(rc);
  if (hipMemsetAsync(ctx->d_flag, 0, sizeof(int), ctx->st) != hipSuccess ||
      hipMemcpyAsync(drp, row_ptr, (q + 1) * 4, hipMemcpyHostToDevice, ctx->st) != hipSuccess ||
      (nnz && (hipMemcpyAsync(dkd, kind, nnz * 4, hipMemcpyHostToDevice, ctx->st) != hipSuccess ||
               hipMemcpyAsync(dix, idx, nnz * 4, hipMemcpyHostToDevice, ctx->st) != hipSuccess ||
               hipMemcpyAsync(dcf, coeff, nnz * 32, hipMemcpyHostToDevice, ctx->st) != hipSuccess)))
    return fail(BPGPU_E_DEVICE);
  circuit_transpose(ctx->st, q, (const uint32_t *)drp, (const uint32_t *)dkd, (const uint32_t *)dix, (const Words8 *)dcf, n_mul, m, ark,
                    c->col_ptr, (uint32_t *)dfill, c->row, c->coeff, ctx->d_flag);
  int bad = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, ctx->d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->st) != hipSuccess ||
      hipStreamSynchronize(ctx->st) != hipSuccess)
    return fail(BPGPU_E_DEVICE);
  if (bad) return fail(BPGPU_E_ARG);
  *out = c;
  return BPGPU_OK;
} catch (const std::bad_alloc &) {   // host-side staging (std::vector): no exception crosses the C ABI
  return BPGPU_E_OOM;
}
int bpgpu_circuit_create(bpgpu_ctx *ctx, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                         const uint8_t *coeff, size_t n_mul, size_t m, bpgpu_circuit **out) {
  return circuit_create_impl(ctx, q, 0, row_ptr, kind, idx, coeff, n_mul, m, out);
}
int bpgpu_circuit_create_ark(bpgpu_ctx *ctx, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                             const uint8_t *coeff_ark, size_t n_mul, size_t m, bpgpu_circuit **out) {
  return circuit_create_impl(ctx, q, 0, row_ptr, kind, idx, coeff_ark, n_mul, m, out, true);
}
int bpgpu_circuit_create_param(bpgpu_ctx *ctx, size_t q, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                               const uint32_t *idx, const uint8_t *coeff, size_t n_mul, size_t m, bpgpu_circuit **out) {
  if (nchi > 8) return BPGPU_E_LEN;
  return circuit_create_impl(ctx, q, nchi, row_ptr, kind, idx, coeff, n_mul, m, out);
}
int bpgpu_circuit_set_gadget_labels(bpgpu_ctx *ctx, bpgpu_circuit *c, const uint8_t *labels) try {
  static std::atomic<uint64_t> next_id{1};
  if (!ctx || !c || !labels || !c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  c->labels.assign(labels, labels + c->nchi * GADGET_LABEL_BYTES);
  c->labels_id = next_id.fetch_add(1);
  return BPGPU_OK;
} catch (const std::bad_alloc &) {
  return BPGPU_E_OOM;
}
// What a device-transcript entry point makes of (circuit, gadget_label argument): with labels attached the argument must be null
// and any nchi goes; without, `unattached_ok` is the entry point's own rule for the one label.  The attached table (host), or null
static const uint8_t *circuit_labels(const bpgpu_circuit *c) { return c->labels.empty() ? nullptr : c->labels.data(); }
static int gadget_label_rule(const bpgpu_circuit *c, const uint8_t *gadget_label, bool unattached_ok) {
  if (circuit_labels(c)) return gadget_label ? BPGPU_E_ARG : BPGPU_OK;
  return unattached_ok ? BPGPU_OK : BPGPU_E_ARG;
}
void bpgpu_circuit_destroy(bpgpu_ctx *ctx, bpgpu_circuit *c) {
  if (!c) return;
  if (ctx) { std::lock_guard<std::mutex> lk(ctx->mu); hipStreamSynchronize(ctx->st); hipStreamSynchronize(ctx->st2); }
  hipFree(c->coeff);     // [coeff | col_ptr | row] is one allocation
  hipFree(c->view_mem);  // the row-major view, if a call ever asked for it
  delete c;
}
static CircuitDev circuit_dev(const bpgpu_circuit *c) {
  CircuitDev d;
  d.col_ptr = c->col_ptr; d.row = c->row; d.coeff = c->coeff;
  d.q = c->q; d.n = c->n; d.m = c->m; d.nnz = c->nnz;
  d.nchi = c->nchi; d.qz = c->q * (1 + c->nchi);
  return d;
}
int bpgpu_flatten_constraints(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *z, uint8_t *wL,
                              uint8_t *wR, uint8_t *wO, uint8_t *wV, uint8_t *wc) {
  if (!ctx || !c || (nb && (!z || (c->n && (!wL || !wR || !wO)) || (c->m && !wV)))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;     // parametric circuits are flattened inside the verification entry points (they need chi)
  if (!nb) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  size_t n = c->n, m = c->m;
  void *dz, *dw, *dzp;
  CK(ws_get(ctx, WS_ARG0, nb * 32, &dz));
  CK(ws_get(ctx, WS_ARG1, nb * (3 * n + m + 1) * 32, &dw));
  CK(ws_get(ctx, WS_ZPOW, nb * (c->q ? c->q : 1) * 9 * 4, &dzp));
  Words8 *w = (Words8 *)dw;
  Words8 *dL = w, *dR = w + nb * n, *dO = w + 2 * nb * n, *dV = w + 3 * nb * n, *dC = w + 3 * nb * n + nb * m;
  CK(flag_reset(ctx));
  CK(h2d(ctx, dz, z, nb * 32));
  scalars_check(ctx->st, (Words8 *)dz, nb, ctx->d_flag);
  flatten(ctx->st, circuit_dev(c), nb, (Words8 *)dz, 8, dL, dR, dO, dV, dC, (int32_t *)dzp);
  return checked_download(ctx, {{wL, dL, nb * n * 32}, {wR, dR, nb * n * 32}, {wO, dO, nb * n * 32}, {wV, dV, nb * m * 32}, {wc, dC, wc ? nb * 32 : 0}});
}

/* ---- Prover::constraints_satisfied (prover.rs:405-409) and a party's half of MpcProver::constraints_satisfied (mpc_prover.rs:538-568):
 * the witnesses of nb provers against the rows of their circuit (k_rows.hip) -------------------------------------------------------- */
// the row-major view of c, built on first use (ctx->mu held).  The build ends with a wait: the number of long rows sizes every later
// launch, and a second context must not read a view that the first one's stream is still writing.
static int circuit_view(bpgpu_ctx *ctx, const bpgpu_circuit *c, RowsDev *out) {
  std::lock_guard<std::mutex> lk(c->view_mu);
  if (!c->view_ready) {
    const CircuitDev cd = circuit_dev(c);
    if (!rows_view_supported(cd)) return BPGPU_E_LEN;
    void *mem = nullptr;
    if (hipMalloc(&mem, rows_view_bytes(cd)) != hipSuccess) { (void)hipGetLastError(); return BPGPU_E_OOM; }
    RowsDev v{};
    const uint32_t *nlong_dev = nullptr;
    uint32_t nlong = 0;
    rows_view_build(ctx->st, cd, mem, &v, &nlong_dev);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nlong, nlong_dev, 4, hipMemcpyDeviceToHost, ctx->st) != hipSuccess ||
        hipStreamSynchronize(ctx->st) != hipSuccess) {
      ctx->err = "building the row-major view of a circuit failed";
      (void)hipFree(mem);
      return BPGPU_E_DEVICE;
    }
    v.nlong = nlong;
    c->view_mem = mem; c->view = v; c->view_ready = true;
  }
  *out = c->view;
  return BPGPU_OK;
}
// the refusals that depend on arguments alone (BPGPU_OK with nb == 0: nothing to do)
static int rows_check(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const void *a_L, const void *a_R, const void *a_O, const void *v,
                      const void *gadget_challenges, const void *out) {
  if (!ctx || !c) return BPGPU_E_ARG;
  if ((c->nchi != 0) != (gadget_challenges != nullptr)) return BPGPU_E_ARG;   // challenges for a numeric circuit, or none for a parametric one
  if (!nb) return BPGPU_OK;
  if (!out || (c->n && (!a_L || !a_R || !a_O)) || (c->m && !v)) return BPGPU_E_ARG;
  return BPGPU_OK;
}
namespace {
struct PoolBlock {   // one pool buffer, given back on the way out (stream-ordered reuse)
  bpgpu_ctx *ctx; void *p = nullptr;
  explicit PoolBlock(bpgpu_ctx *c) : ctx(c) {}
  ~PoolBlock() { pool_release(ctx, p); }
};
struct RowsIo { const void *a_L, *a_R, *a_O, *v, *chi; void *ok, *first_row, *first_gate, *resid; };   // src_dev: all in HBM
}  // namespace
// ctx->mu held, arguments checked, nb > 0.  planes == 1: the check (ok / first_row / first_gate / resid in HBM, the last three optional;
// resid plain canonical); planes == 3: a party's evaluation (resid only: nb x 3 x q, ark form).  Asynchronous but for the one-time
// build of the view.
static int rows_locked(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, int planes, const RowsIo &io, bool src_dev) {
  RowsDev view;
  CK(circuit_view(ctx, c, &view));
  const size_t nv = nb * (size_t)planes, n = c->n, m = c->m, nchi = c->nchi;
  if (!rows_eval_fits(view, nv)) return BPGPU_E_LEN;
  hipStream_t st = ctx->st;
  // staging: [a_L | a_R | a_O | v] (ark in, plain after the conversion), the gadget challenges, the two words per prover
  const size_t nval = 3 * nv * n + nv * m;
  PoolBlock blk(ctx);
  if (!pool_alloc(ctx, &blk.p, (nval + nb * nchi) * 32 + 2 * nv * 4)) return BPGPU_E_OOM;
  Words8 *dL = (Words8 *)blk.p, *dR = dL + nv * n, *dO = dR + nv * n, *dV = dO + nv * n, *dchi = dV + nv * m;
  uint32_t *dbad = (uint32_t *)(dchi + nb * nchi);
  CK(copy_in(ctx, dL, io.a_L, nv * n * 32, src_dev));
  CK(copy_in(ctx, dR, io.a_R, nv * n * 32, src_dev));
  CK(copy_in(ctx, dO, io.a_O, nv * n * 32, src_dev));
  CK(copy_in(ctx, dV, io.v, nv * m * 32, src_dev));
  CK(copy_in(ctx, dchi, io.chi, nb * nchi * 32, src_dev));
  scalars_from_ark(st, dL, dL, nval, ctx->d_flag);                     // in place, as the prover's commit does
  scalars_check(st, dchi, nb * nchi, ctx->d_flag);
  const Words8 *chi = nchi ? dchi : nullptr;
  if (planes == 1) {
    HIPCK(ctx, hipMemsetAsync(dbad, 0xFF, 2 * nb * 4, st));
    rows_eval(st, view, n, m, nchi, nb, 1, dL, dR, dO, dV, chi, dbad, (Words8 *)io.resid);
    rows_gates(st, nb, n, dL, dR, dO, dbad + nb);
    rows_verdict(st, nb, dbad, dbad + nb, (int32_t *)io.ok, (int64_t *)io.first_row, (int64_t *)io.first_gate);
  } else {
    rows_eval(st, view, n, m, nchi, nv, 3, dL, dR, dO, dV, chi, nullptr, (Words8 *)io.resid);
    scalars_to_ark(st, (const Words8 *)io.resid, (Words8 *)io.resid, nv * view.q, ctx->d_flag);
  }
  return launch_ok(ctx);
}
int bpgpu_r1cs_constraints_satisfied_dev(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const void *a_L, const void *a_R, const void *a_O,
                                         const void *v, const void *gadget_challenges, void *ok, void *first_bad_row, void *first_bad_gate,
                                         void *residuals) {
  return noexcept_abi([&]() -> int {
    CK(rows_check(ctx, c, nb, a_L, a_R, a_O, v, gadget_challenges, ok));
    if (!nb) return BPGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    CK(flag_reset(ctx));   // the flag reports on the most recent *_dev call
    return rows_locked(ctx, c, nb, 1, {a_L, a_R, a_O, v, gadget_challenges, ok, first_bad_row, first_bad_gate, residuals}, true);
  });
}
int bpgpu_r1cs_constraints_satisfied(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *a_L, const uint8_t *a_R,
                                     const uint8_t *a_O, const uint8_t *v, const uint8_t *gadget_challenges, int32_t *ok,
                                     int64_t *first_bad_row, int64_t *first_bad_gate, uint8_t *residuals) {
  return noexcept_abi([&]() -> int {
    CK(rows_check(ctx, c, nb, a_L, a_R, a_O, v, gadget_challenges, ok));
    if (!nb) return BPGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    // the results' staging: ok, then the optional ones
    const size_t b_ok = (nb * 4 + 255) / 256 * 256, b_idx = (nb * 8 + 255) / 256 * 256, b_res = residuals ? nb * c->q * 32 : 0;
    PoolBlock out(ctx);
    if (!pool_alloc(ctx, &out.p, b_ok + 2 * b_idx + b_res)) return BPGPU_E_OOM;
    uint8_t *dok = (uint8_t *)out.p, *drow = dok + b_ok, *dgate = drow + b_idx, *dres = dgate + b_idx;
    CK(flag_reset(ctx));
    CK(rows_locked(ctx, c, nb, 1, {a_L, a_R, a_O, v, gadget_challenges, dok, first_bad_row ? drow : nullptr, first_bad_gate ? dgate : nullptr,
                                   residuals ? dres : nullptr}, false));
    return checked_download(ctx, {{ok, dok, nb * 4}, {first_bad_row, drow, first_bad_row ? nb * 8 : 0},
                                  {first_bad_gate, dgate, first_bad_gate ? nb * 8 : 0}, {residuals, dres, b_res}});
  });
}
int bpgpu_mpc_constraints_eval(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                               const uint8_t *v, const uint8_t *gadget_challenges, uint8_t *residuals) {
  return noexcept_abi([&]() -> int {
    CK(rows_check(ctx, c, nb, a_L, a_R, a_O, v, gadget_challenges, residuals));
    if (!nb) return BPGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t b_res = nb * 3 * c->q * 32;
    PoolBlock out(ctx);
    if (!pool_alloc(ctx, &out.p, b_res)) return BPGPU_E_OOM;
    CK(flag_reset(ctx));
    CK(rows_locked(ctx, c, nb, 3, {a_L, a_R, a_O, v, gadget_challenges, nullptr, nullptr, nullptr, out.p}, false));
    return checked_download(ctx, {{residuals, out.p, b_res}});
  });
}

/* ---------------------------------------------------------------- per-proof verification: shape, plan, one function per launch route */
static size_t verify_nvar(const bpgpu_circuit *c, size_t k) { return 11 + c->m + 2 * k; }   // proof points of one proof
// (k < 32) padded_n = 2^k must be next_pow2(n), the first phase n1 of the n multipliers, and the generators must reach that far
static int verify_shape(const bpgpu_circuit *c, const bpgpu_gens *g, size_t n1, size_t k) {
  const size_t np = (size_t)1 << k, n = c->n;
  if (n > np || n1 > n || (np > 1 && n <= np / 2 && n != 0)) return BPGPU_E_LEN;
  return np > g->cap ? BPGPU_E_GENS : BPGPU_OK;
}
namespace {
struct VerifyOperands { const void *points, *scalars, *challenges; void *ok, *mega, *full_sc; };
struct VarRange { size_t lo, hi; };   // a range of one proof's points
// What one call of verify_batch_dev_locked works with, filled once by verify_plan: the sizes, the workspace slots it holds for the
// routes (they take WS_MSM, WS_MSM2 and msm_wp_batch's on top) and what picks the route.
struct VerifyPlan {
  size_t nb, np, nvar;
  const size_t *shard;      // {rank, world} (nb == 1), or nullptr
  VerifyDims d;
  void *dpts, *dfix, *dvar, *dzp, *dvres, *dfres, *dstr;   // WS_VPTS, WS_VFIX, WS_VVAR, WS_ZPOW, WS_VVRES, WS_VFRES, WS_STRAUS
  int32_t *dbadsc, *dbadpt; // WS_VBITS: per-proof canonicity bits of the scalar assembly (every entry is written by the kernel: no
                            // reset) | per-proof malformed-point bits of the Straus / separate-launch routes
  bool one_chunk;           // the generator half is a single chunk of the fixed-base MSM ...
  bool fused_fixed;         // ... and rides in the window-parallel back launch: <= 16 384 (generator, window) pairs per proof
  size_t fparts;            // partial sums per proof it leaves there (nb x parts when it is walked a proof per lane: BPGPU_OPT_FIXED_CHUNK_GENS)
  bool no_fuse, no_wp;      // BPGPU_OPT_VERIFY_NO_FUSE != 0, BPGPU_OPT_VERIFY_WINDOW_PARALLEL == 0
  int vnp;                  // Straus routes: points per lane, sharing one doubling chain (BPGPU_OPT_VERIFY_STRAUS_NP) ...
  size_t lanes, rem, nres;  // ... lanes per proof, leftover points (one per lane), sums per proof = lanes + rem
};
}
// shard = {rank, world} (nb == 1): this rank's share of ONE proof's mega_check -- the generators and the proof points of its
// slice; `mega` receives the partial sum (the ranks all-gather and add them: SURVEY 8e.2), `ok` says whether the PARTIAL is the identity
static int verify_plan(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k, const void *chi,
                       const size_t *shard, VerifyPlan &p) {
  if (k >= 32) return BPGPU_E_LEN;
  if (shard && (nb != 1 || !shard[1] || shard[0] >= shard[1])) return BPGPU_E_ARG;
  if ((c->nchi != 0) != (chi != nullptr)) return BPGPU_E_ARG;   // a parametric circuit needs its gadget challenges, and only it
  CK(verify_shape(c, g, n1, k));
  if (!nb) return BPGPU_OK;     // (nothing is planned: the caller returns before any HIP call)
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)1 << k, nvar = verify_nvar(c, k), nfix = 2 + 2 * np;
  p.nb = nb; p.np = np; p.nvar = nvar; p.shard = shard;
  CK(ws_get(ctx, WS_VPTS, nb * nvar * sizeof(AffDev), &p.dpts));
  CK(ws_get(ctx, WS_VFIX, nb * nfix * 32, &p.dfix));
  CK(ws_get(ctx, WS_VVAR, nb * nvar * 32, &p.dvar));
  p.d = VerifyDims{nb, n1, c->n, np, k, c->m, (const Words8 *)chi, (size_t)ctx->opt[BPGPU_OPT_VS_LARGE_MIN]};
  CK(ws_get(ctx, WS_ZPOW, verify_scalars_scratch_ints(circuit_dev(c), p.d) * 4, &p.dzp));
  CK(ws_get(ctx, WS_VVRES, nb * nvar * sizeof(JacRaw), &p.dvres));
  p.one_chunk = fixed_msm_chunks(g->c, np, nb) == 1;
  p.fused_fixed = p.one_chunk && verify_wp_supported(nb, nvar, g->c, np);
  p.fparts = 1;
  if (p.fused_fixed) {
    VerifyWp vt{};
    vt.nb = nb; vt.latency_mode = ctx->latency_mode;
    wp_options(ctx, vt);
    p.fparts = verify_wp_fixed_parts(vt, np);
  }
  CK(ws_get(ctx, WS_VFRES, nb * p.fparts * sizeof(JacRaw), &p.dfres));
  CK(straus_ws(ctx, 4, nb * nvar, &p.dstr));
  CK(ws_get(ctx, WS_VBITS, 2 * nb * sizeof(int32_t), (void **)&p.dbadsc));
  p.dbadpt = p.dbadsc + nb;
  p.no_fuse = ctx->opt[BPGPU_OPT_VERIFY_NO_FUSE] != 0;
  p.no_wp = ctx->opt[BPGPU_OPT_VERIFY_WINDOW_PARALLEL] == 0;
  const int vnp_opt = (int)ctx->opt[BPGPU_OPT_VERIFY_STRAUS_NP];
  p.vnp = vnp_opt < 1 ? 1 : (vnp_opt > 4 ? 4 : vnp_opt);
  p.lanes = nvar / p.vnp; p.rem = nvar - p.lanes * p.vnp; p.nres = p.lanes + p.rem;
  return BPGPU_OK;
}
// A shard's share of the proof: the other ranks' generator and proof-point scalars are zeroed (a zero digit costs the table-lookup
// lanes nothing but the walk).  -> this rank's range of the proof points (all of them without a shard)
static VarRange verify_shard_mask(bpgpu_ctx *ctx, const VerifyPlan &p) {
  VarRange v{0, p.nvar};
  if (p.shard) {
    size_t slo, shi;
    shard_bounds(p.np, p.shard[0], p.shard[1], &slo, &shi);
    shard_bounds(p.nvar, p.shard[0], p.shard[1], &v.lo, &v.hi);
    shard_mask(ctx->st, (Words8 *)p.dfix, p.np, slo, shi, p.shard[0] == 0, (Words8 *)p.dvar, p.nvar, v.lo, v.hi);
  }
  return v;
}
// the generator half on the second stream, beside what ctx->st runs until side_join (part_slot: its chunk partials)
static int verify_gens_on_side(bpgpu_ctx *ctx, const bpgpu_gens *g, const VerifyPlan &p, WsSlot part_slot = WS_MSM, int lpm = 0) {
  CK(side_fork(ctx));
  { ProfScope ps(ctx, 1, ctx->st2);
    CK(msm_gens_dev(ctx, g, p.nb, p.np, (const uint32_t *)p.dfix, (JacRaw *)p.dfres, ctx->st2, part_slot, lpm)); }
  return side_done(ctx);
}
// Default route: window-parallel variable-base part -- front [tables | inversion pass], scalars, windows, groups,
// back [Horner | fixed-base MSMs], verdict (k_ec.hip).  Every launch is on ctx->st.
// The generator half rides in the back launch when it is small (p.fused_fixed); otherwise -- few proofs of a mid-size circuit, or a
// table window the fused kernel is not built for -- it is its own chunked launch ahead of the Horner pass.
static int verify_route_wp(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const VerifyPlan &p, const VerifyOperands &o) {
  const size_t nb = p.nb, np = p.np, nvar = p.nvar;
  const VerifyDims &d = p.d;
  void *dwp;
  CK(ws_get(ctx, WS_MSM, verify_wp_scratch_bytes(nb, nvar), &dwp));
  VerifyWp v{(const AffDev *)o.points, nb, nvar, dwp, ctx->d_flag, p.dbadsc, ctx->latency_mode, false, (int)ctx->opt[BPGPU_OPT_TABLE_NP]};
  wp_options(ctx, v);
  if (!verify_wp_layout_fits(v)) { ctx->err = "internal: window-parallel scratch layout exceeds its buffer (verify)"; return BPGPU_E_DEVICE; }
  int32_t *aux = nullptr; size_t aux_stride = 0;
  const bool fuse_prep = verify_scalars_aux(circuit_dev(c), d, (int32_t *)p.dzp, &aux, &aux_stride);
  const bool fast = fuse_prep && verify_scalars_fast_shape(circuit_dev(c), d);   // wave-sized proofs: the serial part of the assembly in the front launch's lanes
  { ProfScope ps(ctx, 8, ctx->st);
    verify_wp_front_launch(ctx->st, v, d, (const Words8 *)o.challenges, aux, aux_stride, fuse_prep, fast ? (const Words8 *)o.scalars : nullptr,
                           fast ? (Words8 *)p.dfix : nullptr, fast ? (Words8 *)p.dvar : nullptr, fast ? (Words8 *)o.full_sc : nullptr); }
  { ProfScope ps(ctx, 0, ctx->st);
    verify_scalars(ctx->st, circuit_dev(c), d, (const Words8 *)o.challenges, (const Words8 *)o.scalars, (Words8 *)p.dfix,
                   (Words8 *)p.dvar, (Words8 *)o.full_sc, (int32_t *)p.dzp, ctx->d_flag, p.dbadsc, fuse_prep, fast); }
  verify_shard_mask(ctx, p);   // a small proof: the other ranks' terms are simply zeroed (every rank walks all the points)
  // Latency mode with a second stream: the generator half needs nothing but the scalars, so it runs BESIDE the window sums,
  // the first Horner stage and the Horner pass instead of sharing the back launch with the wave-per-proof Horner rows (which
  // then have the SIMDs to themselves): a lone batch's chain loses the ~0.15 ms the two halves spent taking turns.
  const bool side = p.fused_fixed && ctx->latency_mode && ctx->st2 != ctx->st && !p.shard;
  const bool in_back = p.fused_fixed && !side;
  if (side) CK(verify_gens_on_side(ctx, g, p, WS_MSM2, 64));
  { ProfScope ps(ctx, 7, ctx->st); verify_wp_windows(ctx->st, v, (const uint32_t *)p.dvar); }
  { ProfScope ps(ctx, 9, ctx->st); verify_wp_groups(ctx->st, v); }
  if (!p.fused_fixed) { ProfScope ps(ctx, 1, ctx->st);
    CK(msm_gens_dev(ctx, g, nb, np, (const uint32_t *)p.dfix, (JacRaw *)p.dfres, ctx->st, WS_MSM2)); }
  { ProfScope ps(ctx, 10, ctx->st);
    verify_wp_back(ctx->st, v, g->c, in_back ? g->table : nullptr, np, g->cap, (const uint32_t *)p.dfix, (2 + 2 * np) * 8, (JacRaw *)p.dfres); }
  if (side) CK(side_join(ctx));
  { ProfScope ps(ctx, 11, ctx->st);
    verify_wp_verdict(ctx->st, v, (const JacRaw *)p.dfres, (int32_t *)o.ok, (Words8 *)o.mega, in_back ? p.fparts : 1); }
  return BPGPU_OK;
}
// The head of the three routes below: scalar assembly (canonicity of the scalars and challenges is checked inside verify_scalars),
// then the shard's mask.  -> this rank's range of the proof points
static int verify_straus_scalars(bpgpu_ctx *ctx, const bpgpu_circuit *c, const VerifyPlan &p, const VerifyOperands &o, VarRange *var) {
  const size_t nb = p.nb;
  int32_t *dbadpt = p.dbadpt;
  HIPCK(ctx, hipMemsetAsync(dbadpt, 0, nb * sizeof(int32_t), ctx->st));
  { ProfScope ps(ctx, 0, ctx->st);
    verify_scalars(ctx->st, circuit_dev(c), p.d, (const Words8 *)o.challenges, (const Words8 *)o.scalars, (Words8 *)p.dfix,
                   (Words8 *)p.dvar, (Words8 *)o.full_sc, (int32_t *)p.dzp, ctx->d_flag, p.dbadsc); }
  *var = verify_shard_mask(ctx, p);
  return BPGPU_OK;
}
// ... and their tail: the nres sums of a proof's points + its generator half -> ok, mega
static void verify_finalize_launch(bpgpu_ctx *ctx, const VerifyPlan &p, const VerifyOperands &o, size_t nres) {
  ProfScope ps(ctx, 4, ctx->st);
  verify_finalize(ctx->st, (JacRaw *)p.dvres, nres, (JacRaw *)p.dfres, p.nb, (int32_t *)o.ok, (Words8 *)o.mega, p.dbadsc, p.dbadpt);
}
// ONE large proof (the 2^14-shuffle: 32 809 proof points): its variable-base half as 16-point groups through the window-
// parallel launches (msm_wp_batch) instead of a Straus lane per 4 points, a one-point remainder launch and a 256-deep
// serial sum (1.9 + 0.9 + 1.15 ms -> 0.8 ms); the generator half runs on the second stream.  Only this rank's slice `var` of the
// points is touched at all.  *done = false: msm_wp_batch declined, the Straus routes take over.
static int verify_route_large(bpgpu_ctx *ctx, const bpgpu_gens *g, const VerifyPlan &p, const VerifyOperands &o, VarRange var, bool *done) {
  void *dvres = p.dvres;
  CK(verify_gens_on_side(ctx, g, p, WS_MSM2));
  *done = false;
  { ProfScope ps(ctx, 3, ctx->st);
    if (var.hi > var.lo) CK(msm_wp_batch(ctx, 1, var.hi - var.lo, (const uint8_t *)p.dvar + var.lo * 32, (const uint8_t *)o.points + var.lo * 64, false,
                                         (JacRaw *)dvres, done, (int *)p.dbadpt, (size_t)1 << 16));
    else { HIPCK(ctx, hipMemsetAsync(dvres, 0, sizeof(JacRaw), ctx->st)); *done = true; }    // (zero limbs = the identity)
  }
  CK(side_join(ctx));
  if (*done) verify_finalize_launch(ctx, p, o, 1);
  return BPGPU_OK;
}
// Straus lanes over `npl` points each of every proof's points from `first` on (npl = p.vnp: the p.lanes full lanes; 1: the leftover
// points).  Lanes are ROLE-major (lane = role * nb + proof): the 64 lanes of a wave hold the same proof element of 64 proofs, so the
// identity points of 1-phase proofs (A_I2, A_O2, S2) are skipped wave-uniformly inside k_straus.
// bad != nullptr: pts are the ABI bytes, validated and converted in the launch
static StrausArgs verify_straus_args(const VerifyPlan &p, const AffDev *pts, size_t first, int npl, int *bad = nullptr) {
  StrausArgs a{};
  for (int j = 0; j < npl; j++) {
    a.pts[j] = pts + first + j * p.lanes; a.pt_stride[j] = p.nvar; a.pt_outer[j] = 1;
    a.sc[j] = (uint32_t *)p.dvar + (first + j * p.lanes) * 8; a.sc_stride[j] = p.nvar * 8; a.sc_outer[j] = 8;
  }
  a.inner = p.nb; a.out_outer = 1; a.out_stride = p.nres;
  if (bad) { a.from_boundary = 1; a.bad = bad; a.bad_inner = p.dbadpt; }
  return a;
}
// One launch for both halves of the MSM, reading the proof points straight from the ABI bytes (+ one for the leftover points).
// *done = false: this (vnp, c, size) combination has no fused kernel, the separate launches take over.
static int verify_route_fused(bpgpu_ctx *ctx, const bpgpu_gens *g, const VerifyPlan &p, const VerifyOperands &o, bool *done) {
  const size_t nb = p.nb, np = p.np;
  *done = false;
  if (!p.lanes) return BPGPU_OK;
  { ProfScope ps(ctx, 6, ctx->st);
    *done = verify_msm_fused(ctx->st, p.vnp, verify_straus_args(p, (const AffDev *)o.points, 0, p.vnp, ctx->d_flag), (JacRaw *)p.dvres, nb * p.lanes,
                             p.dstr, g->c, g->table, np, g->cap, (const uint32_t *)p.dfix, (2 + 2 * np) * 8, (JacRaw *)p.dfres, nb);
    if (*done && p.rem) {
      void *dstr2;
      CK(ws_get(ctx, WS_MSM, straus_scratch_bytes(1, nb * p.rem), &dstr2));
      straus(ctx->st, 1, verify_straus_args(p, (const AffDev *)o.points, p.vnp * p.lanes, 1, ctx->d_flag), (JacRaw *)p.dvres + p.lanes, nb * p.rem, dstr2);
    }
  }
  if (*done) verify_finalize_launch(ctx, p, o, p.nres);
  return BPGPU_OK;
}
// Separate launches: the fixed-base part on st2 while st converts the proof points and runs their Straus lanes
static int verify_route_separate(bpgpu_ctx *ctx, const bpgpu_gens *g, const VerifyPlan &p, const VerifyOperands &o) {
  const size_t nb = p.nb, nvar = p.nvar;
  const AffDev *dpts = (const AffDev *)p.dpts;
  CK(verify_gens_on_side(ctx, g, p));
  { ProfScope ps(ctx, 2, ctx->st);
    points_from_boundary(ctx->st, (const Words8 *)o.points, (AffDev *)p.dpts, nb * nvar, ctx->d_flag, p.dbadpt, nvar); }
  { ProfScope ps(ctx, 3, ctx->st);
    if (p.lanes) straus(ctx->st, p.vnp, verify_straus_args(p, dpts, 0, p.vnp), (JacRaw *)p.dvres, nb * p.lanes, p.dstr);
    if (p.rem) straus(ctx->st, 1, verify_straus_args(p, dpts, p.vnp * p.lanes, 1), (JacRaw *)p.dvres + p.lanes, nb * p.rem, p.dstr); }
  CK(side_join(ctx));
  verify_finalize_launch(ctx, p, o, p.nres);
  return BPGPU_OK;
}
static int verify_batch_dev_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                   size_t k, const void *points, const void *scalars, const void *challenges,
                                   void *ok, void *mega, void *full_sc, const void *chi = nullptr, const size_t *shard = nullptr) {
  VerifyPlan p;
  CK(verify_plan(ctx, g, c, nb, n1, k, chi, shard, p));
  if (!nb) return BPGPU_OK;
  const VerifyOperands o{points, scalars, challenges, ok, mega, full_sc};
  const bool wp = !p.no_fuse && !p.no_wp;
  // The window kernel walks a proof's points serially in every window lane: up to 256 proof points, unless the generator half
  // rides along (the 2^14-shuffle's 32 809 take the routes below)
  if (wp && p.nvar && (p.fused_fixed || p.nvar <= 256)) { CK(verify_route_wp(ctx, g, c, p, o)); return launch_ok(ctx); }
  VarRange var;
  CK(verify_straus_scalars(ctx, c, p, o, &var));
  bool done = false;
  if (wp && nb == 1 && p.nvar <= ((size_t)1 << 16)) CK(verify_route_large(ctx, g, p, o, var, &done));
  if (!done && !p.no_fuse && p.one_chunk) CK(verify_route_fused(ctx, g, p, o, &done));
  if (!done) CK(verify_route_separate(ctx, g, p, o));
  return launch_ok(ctx);
}
int bpgpu_r1cs_verify_batch_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                size_t k, const void *points, const void *scalars, const void *challenges,
                                void *ok, void *mega, void *full_sc) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !ok))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_batch_dev_locked(ctx, g, c, nb, n1, k, points, scalars, challenges, ok, mega, full_sc);
}
/* ONE proof's mega_check split over the GPUs of a node by term range (BASELINE configs[3]: 98 347 terms): this
 * rank's partial point.  Every rank runs the (cheap, O(n)) scalar assembly in full and the MSM over its share only. */
int bpgpu_r1cs_verify_shard(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t n1, size_t k, const uint8_t *points,
                            const uint8_t *scalars, const uint8_t *challenges, const uint8_t *gadget_challenges, size_t rank, size_t world,
                            uint8_t partial_xy[64]) {
  if (!ctx || !g || !c || !points || !scalars || !challenges || !partial_xy || !world || rank >= world) return BPGPU_E_ARG;
  if ((c->nchi != 0) != (gadget_challenges != nullptr)) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t nvar = verify_nvar(c, k);
  void *dP, *dS, *dC, *dok, *dmega, *dchi = nullptr;
  CK(ws_get(ctx, WS_ARG0, nvar * 64, &dP));
  CK(ws_get(ctx, WS_ARG1, 5 * 32, &dS));
  CK(ws_get(ctx, WS_ARG2, (6 + k) * 32, &dC));
  CK(ws_get(ctx, WS_ARG3, 4, &dok));
  CK(ws_get(ctx, WS_ARG4, 64, &dmega));
  if (c->nchi) { CK(ws_get(ctx, WS_CHI, c->nchi * 32, &dchi)); CK(h2d(ctx, dchi, gadget_challenges, c->nchi * 32)); }
  CK(flag_reset(ctx));
  CK(h2d(ctx, dP, points, nvar * 64));
  CK(h2d(ctx, dS, scalars, 5 * 32));
  CK(h2d(ctx, dC, challenges, (6 + k) * 32));
  if (dchi) scalars_check(ctx->st, (const Words8 *)dchi, c->nchi, ctx->d_flag);
  const size_t shard[2] = {rank, world};
  void *dbits;                       // the proof's malformed-scalar | malformed-point bits (verify_batch_dev_locked's, nb = 1)
  CK(ws_get(ctx, WS_VBITS, 2 * sizeof(int32_t), &dbits));
  HIPCK(ctx, hipMemsetAsync(dbits, 0, 2 * sizeof(int32_t), ctx->st));
  CK(verify_batch_dev_locked(ctx, g, c, 1, n1, k, dP, dS, dC, dok, dmega, nullptr, dchi, shard));
  // A malformed operand (off-curve / non-canonical point, non-canonical scalar or challenge) is seen only by the rank whose share
  // holds it: the context flag, or -- on the large-proof route, which validates this rank's slice of the points into the proof's
  // own bits -- the per-proof bits of WS_VBITS (scalars | points).  The verdict must be COLLECTIVE: this rank returns
  // BPGPU_OK with the poison encoding (64 bytes 0xFF: not a point), and bpgpu_points_sum over the gathered partials fails with
  // BPGPU_E_ARG on every rank alike.  (An error code on one rank only would leave the others waiting in their all-gather.)
  int bad = 0;
  CK(flag_read(ctx, &bad));
  int32_t bits[2] = {0, 0};
  CK(d2h(ctx, bits, dbits, sizeof bits));
  CK(d2h(ctx, partial_xy, dmega, 64));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  if (bad || bits[0] || bits[1]) memset(partial_xy, 0xFF, 64);
  return BPGPU_OK;
}
// bpgpu_r1cs_verify_batch(_param) after their argument checks: the operands go up, the verdicts come back
static int verify_batch_host(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                             const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *gadget_challenges,
                             int32_t *ok, uint8_t *mega, uint8_t *msm_scalars) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)1 << k, nvar = verify_nvar(c, k), nterms = nvar + 2 + 2 * np;   // proof points + B, B_blinding, G, H
  void *dP, *dS, *dC, *dok, *dmega, *dfull = nullptr, *dchi = nullptr;
  CK(ws_get(ctx, WS_ARG0, nb * nvar * 64, &dP));
  CK(ws_get(ctx, WS_ARG1, nb * 5 * 32, &dS));
  CK(ws_get(ctx, WS_ARG2, nb * (6 + k) * 32, &dC));
  CK(ws_get(ctx, WS_ARG3, nb * 4, &dok));
  CK(ws_get(ctx, WS_ARG4, nb * 64, &dmega));
  if (msm_scalars) CK(ws_get(ctx, WS_ARG5, nb * nterms * 32, &dfull));
  if (c->nchi && gadget_challenges) { CK(ws_get(ctx, WS_CHI, nb * c->nchi * 32, &dchi)); CK(h2d(ctx, dchi, gadget_challenges, nb * c->nchi * 32)); }
  CK(h2d(ctx, dP, points, nb * nvar * 64));
  CK(h2d(ctx, dS, scalars, nb * 5 * 32));
  CK(h2d(ctx, dC, challenges, nb * (6 + k) * 32));
  // a malformed proof (off-curve / non-canonical point, non-canonical scalar or challenge) is rejected on its own:
  // ok[p] = 0, the other verdicts stand (the reference's per-proof FormatError / VerificationError); so is a proof with a
  // non-canonical gadget challenge
  void *dchibad = nullptr;
  if (dchi) {
    CK(ws_get(ctx, WS_PROOF_BAD, nb * 4, &dchibad));
    HIPCK(ctx, hipMemsetAsync(dchibad, 0, nb * 4, ctx->st));
    scalars_check_proof(ctx->st, (const Words8 *)dchi, nb * c->nchi, c->nchi, ctx->d_flag, (int32_t *)dchibad);
  }
  CK(verify_batch_dev_locked(ctx, g, c, nb, n1, k, dP, dS, dC, dok, mega ? dmega : nullptr, dfull, dchi));
  if (dchibad) and_not(ctx->st, (int32_t *)dok, (const int32_t *)dchibad, nb);
  CK(d2h(ctx, ok, dok, nb * 4));
  if (mega) CK(d2h(ctx, mega, dmega, nb * 64));
  if (msm_scalars) CK(d2h(ctx, msm_scalars, dfull, nb * nterms * 32));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
int bpgpu_r1cs_verify_batch(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                            size_t k, const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges,
                            int32_t *ok, uint8_t *mega, uint8_t *msm_scalars) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !ok))) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  return verify_batch_host(ctx, g, c, nb, n1, k, points, scalars, challenges, nullptr, ok, mega, msm_scalars);
}

/* A STREAM of verification batches in one call: the proofs are cut into batches of `batch` proofs (default 1024) that take turns
 * on the context's ring of lanes (child contexts: a stream and a set of workspaces each), so that the six-launch chains of
 * ~20 batches overlap on the GPU -- what a caller otherwise builds out of twenty contexts.  The lanes fork from ctx->st (inputs
 * uploaded asynchronously on it are visible) and are joined back into it. */
static int stream_lanes(bpgpu_ctx *ctx, size_t want) {
  if (!ctx->lane_ev) HIPCK(ctx, hipEventCreateWithFlags(&ctx->lane_ev, hipEventDisableTiming));
  while (ctx->lanes.size() < want) {
    bpgpu_ctx *l = nullptr;
    int rc = ctx_create(ctx->device, true, &l);
    if (rc) return rc;
    try { ctx->lanes.push_back(l); } catch (const std::bad_alloc &) { bpgpu_destroy(l); return BPGPU_E_OOM; }
  }
  for (bpgpu_ctx *l : ctx->lanes) {   // the lanes follow their parent's settings
    for (int i = 0; i < BPGPU_OPT_COUNT; i++) l->opt[i] = ctx->opt[i];
    l->latency_mode = false;          // (a stream call is the pipelined case by definition)
    l->horner_group = ctx->horner_group;
    l->prof = ctx->prof; l->prof_mask = ctx->prof_mask;
  }
  return BPGPU_OK;
}
static int lanes_fork(bpgpu_ctx *ctx, size_t nl) {
  HIPCK(ctx, hipEventRecord(ctx->lane_ev, ctx->st));
  for (size_t l = 0; l < nl; l++) HIPCK(ctx, hipStreamWaitEvent(ctx->lanes[l]->st, ctx->lane_ev, 0));
  return BPGPU_OK;
}
// the join runs on the way out of an error (rc) too: the batches already submitted keep running, and nothing the caller does next
// on this context may overtake them: ctx->st -- and with it bpgpu_sync / the caller's next call -- waits for every lane
static int lanes_join(bpgpu_ctx *ctx, size_t nl, int rc, const char *what) {
  for (size_t l = 0; l < nl; l++)
    if (hipEventRecord(ctx->lanes[l]->ev1, ctx->lanes[l]->st) != hipSuccess || hipStreamWaitEvent(ctx->st, ctx->lanes[l]->ev1, 0) != hipSuccess)
      if (rc == BPGPU_OK) { ctx->err = std::string(what) + ": joining the lanes failed"; rc = BPGPU_E_DEVICE; }
  return rc;
}
// page-locked staging for the verdicts of a host-memory stream or screened call (grow-only): an asynchronous copy into the caller's
// (pageable) array would make every batch's download a host-side wait for its lane -- and serialise the lanes
static int pinned_verdicts(bpgpu_ctx *ctx, size_t nb) {
  if (ctx->pinned_cap < nb * 4) {
    if (ctx->pinned) { HIPCK(ctx, hipStreamSynchronize(ctx->st)); (void)hipHostFree(ctx->pinned); ctx->pinned = nullptr; ctx->pinned_cap = 0; }
    HIPCK(ctx, hipHostMalloc(&ctx->pinned, nb * 4 + nb, hipHostMallocDefault));
    ctx->pinned_cap = nb * 4 + nb;
  }
  return BPGPU_OK;
}
static int verify_stream_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, uint8_t *ok, int on_host) {
  // on_host: 0 = operands and verdicts resident; 1 = pageable host memory (staged copies on the lane's stream); 2 = device-mapped
  // page-locked host memory (one fetch launch per batch, verdicts written in place)
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t batch = (size_t)ctx->opt[BPGPU_OPT_STREAM_BATCH], nlanes_opt = (size_t)ctx->opt[BPGPU_OPT_STREAM_LANES];
  const size_t nchunks = (nb + batch - 1) / batch, nl = nchunks < nlanes_opt ? nchunks : nlanes_opt;
  CK(stream_lanes(ctx, nl));
  const size_t nvar = verify_nvar(c, k), nch = 6 + k;
  CK(lanes_fork(ctx, nl));
  int rc = BPGPU_OK;
  for (size_t ci = 0; ci < nchunks && rc == BPGPU_OK; ci++) {
    bpgpu_ctx *ln = ctx->lanes[ci % nl];
    const size_t lo = ci * batch, cnt = nb - lo < batch ? nb - lo : batch;
    const uint8_t *P = points + lo * nvar * 64, *S = scalars + lo * 5 * 32, *Cc = challenges + lo * nch * 32;
    uint8_t *O = ok + lo * 4;
    if (on_host == 2) {
      void *dP, *dS, *dC;
      if (!(rc = ws_get(ln, WS_ARG0, batch * nvar * 64, &dP)) && !(rc = ws_get(ln, WS_ARG1, batch * 5 * 32, &dS)) && !(rc = ws_get(ln, WS_ARG2, batch * nch * 32, &dC))) {
        hipLaunchKernelGGL(k_fetch3, dim3(64), dim3(256), 0, ln->st, (const uint4 *)P, (uint4 *)dP, cnt * nvar * 4, (const uint4 *)S, (uint4 *)dS, cnt * 10,
                           (const uint4 *)Cc, (uint4 *)dC, cnt * nch * 2);
        rc = verify_batch_dev_locked(ln, g, c, cnt, n1, k, dP, dS, dC, O, nullptr, nullptr);
      }
    } else if (on_host) {       // operands and verdicts in pageable host memory: staged through the lane's own buffers
      void *dP, *dS, *dC, *dok;
      (void)((rc = ws_get(ln, WS_ARG0, batch * nvar * 64, &dP)) || (rc = ws_get(ln, WS_ARG1, batch * 5 * 32, &dS)) ||
             (rc = ws_get(ln, WS_ARG2, batch * nch * 32, &dC)) || (rc = ws_get(ln, WS_ARG3, batch * 4, &dok)) ||
             (rc = h2d(ln, dP, P, cnt * nvar * 64)) || (rc = h2d(ln, dS, S, cnt * 5 * 32)) || (rc = h2d(ln, dC, Cc, cnt * nch * 32)) ||
             (rc = verify_batch_dev_locked(ln, g, c, cnt, n1, k, dP, dS, dC, dok, nullptr, nullptr)) ||
             (rc = d2h(ln, O, dok, cnt * 4)));
    } else rc = verify_batch_dev_locked(ln, g, c, cnt, n1, k, P, S, Cc, O, nullptr, nullptr);
    if (rc) ctx->err = ln->err;
  }
  return lanes_join(ctx, nl, rc, "bpgpu_r1cs_verify_stream");
}
int bpgpu_r1cs_verify_stream_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                 const void *points_dev, const void *scalars_dev, const void *challenges_dev, void *ok_dev) {
  if (!ctx || !g || !c || (nb && (!points_dev || !scalars_dev || !challenges_dev || !ok_dev))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_stream_locked(ctx, g, c, nb, n1, k, (const uint8_t *)points_dev, (const uint8_t *)scalars_dev,
                              (const uint8_t *)challenges_dev, (uint8_t *)ok_dev, 0);
}
int bpgpu_r1cs_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                             const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, int32_t *ok) {
  return bpgpu_internal_verify_stream(ctx, g, c, nb, n1, k, points, scalars, challenges, ok, 1);
}
// in_place_ok = 0: page-locked operands take the staged copies as well (bpgpu_internal.h: the pool decides per slot)
__attribute__((visibility("hidden"))) int bpgpu_internal_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                                                       size_t n1, size_t k, const uint8_t *points, const uint8_t *scalars,
                                                                       const uint8_t *challenges, int32_t *ok, int in_place_ok) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !ok))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  CK(pinned_verdicts(ctx, nb));
  // Operands in PAGE-LOCKED host memory (bpgpu_host_alloc, hipHostMalloc, hipHostRegister) are fetched by ONE kernel launch per batch
  // on its lane (k_fetch3: wide coalesced reads over the bus -- 2 080 bytes per proof, 8 GB/s at 4 M proofs/s) and the verdicts are
  // written straight into the page-locked staging.  No copy command is enqueued at all: the per-batch H2D / D2H copies on 20 lanes
  // (four DMA commands and as many cross-engine dependencies per 1024 proofs) held the host-memory stream at 2-3 M/s against 4.1
  // resident; reading the operands in place from the chain's own kernels put bus latency on its latency-bound links (3.4 M/s).
  // Pageable operands take the staged copies on each lane's stream.
  const void *dpts = in_place_ok ? host_device_alias(points) : nullptr, *dsc = host_device_alias(scalars), *dch = host_device_alias(challenges);
  const void *dok = host_device_alias(ctx->pinned);
  if (dpts && dsc && dch && dok)
    CK(verify_stream_locked(ctx, g, c, nb, n1, k, (const uint8_t *)dpts, (const uint8_t *)dsc, (const uint8_t *)dch, (uint8_t *)dok,
                            (((uintptr_t)dpts | (uintptr_t)dsc | (uintptr_t)dch) & 15) ? 0 : 2));   // (16-byte words; unaligned buffers are read in place)
  else
    CK(verify_stream_locked(ctx, g, c, nb, n1, k, points, scalars, challenges, (uint8_t *)ctx->pinned, 1));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  memcpy(ok, ctx->pinned, nb * 4);
  return BPGPU_OK;
}

/* ---------------------------------------------------------------- Verifier::verify with the transcript on the device */
// the transcript half: schedule (cached per context) + k_verify_transcript.  *chp = the challenges (challenges_out or a workspace),
// *dbad = per-proof "a validated point is the identity" flags, *dchi = the gadget challenges of a parametric circuit (or null)
static int fs_transcript_locked(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, size_t k, const void *init_states, const void *points,
                                const void *scalars, void *challenges_out, const uint8_t *gadget_label, void *chi_out, Words8 **chp,
                                void **dbad_out, void **dchi_out) try {
  if (k >= 32) return BPGPU_E_LEN;
  // without attached labels: one gadget challenge label per schedule
  CK(gadget_label_rule(c, gadget_label, !(c->nchi > 1 || (c->nchi == 1 && !gadget_label))));
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t m = c->m, np = (size_t)1 << k, nchi = c->nchi;
  const uint8_t *labels = circuit_labels(c);
  const size_t label_id = labels ? c->labels_id : 0, cap = transcript_schedule_max(m, k, nchi);
  void *dsteps, *dch, *dbad, *dchi = nullptr;
  if (nchi) { if (chi_out) dchi = chi_out; else CK(ws_get(ctx, WS_CHI, nb * nchi * 32, &dchi)); }
  CK(ws_get(ctx, WS_SCHED, (cap + gadget_label_slots(nchi)) * sizeof(TrStep) + 64, &dsteps));
  CK(ws_get(ctx, WS_FS_CH, nb * (6 + k) * 32, &dch));
  CK(ws_get(ctx, WS_PROOF_BAD, nb * 4, &dbad));
  if (ctx->sched_key[0] != m || ctx->sched_key[1] != k || ctx->sched_key[2] != np + (nchi << 40) || ctx->sched_key[3] != label_id) {
    // the steps, and behind them (at step `cap`) the circuit's label table, if it has one: ONE upload
    std::vector<TrStep> steps(cap + gadget_label_slots(nchi));
    ctx->sched_len = transcript_schedule(steps.data(), m, k, np, nchi);
    size_t up = (size_t)ctx->sched_len;
    if (labels) { memcpy(steps.data() + cap, labels, nchi * GADGET_LABEL_BYTES); up = steps.size(); }
    ctx->sched_key[0] = (size_t)-1;              // (nothing resident if the upload fails)
    HIPCK(ctx, hipMemcpyAsync(dsteps, steps.data(), up * sizeof(TrStep), hipMemcpyHostToDevice, ctx->st));
    HIPCK(ctx, hipStreamSynchronize(ctx->st));   // `steps` is a local
    ctx->sched_key[0] = m; ctx->sched_key[1] = k; ctx->sched_key[2] = np + (nchi << 40); ctx->sched_key[3] = label_id;
  }
  *chp = challenges_out ? (Words8 *)challenges_out : (Words8 *)dch;
  *dbad_out = dbad;
  *dchi_out = dchi;
  ProfScope ps(ctx, 5, ctx->st);
  verify_transcript(ctx->st, nb, m, k, (const TrStep *)dsteps, ctx->sched_len, (const Words8 *)init_states,
                    (const Words8 *)points, (const Words8 *)scalars, *chp, (int32_t *)dbad, gadget_label, (Words8 *)dchi, nchi,
                    labels ? (const uint8_t *)((const TrStep *)dsteps + cap) : nullptr);
  return BPGPU_OK;
} catch (const std::bad_alloc &) {   // host-side staging (std::vector): no exception crosses the C ABI
  return BPGPU_E_OOM;
}
static int verify_fs_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                            const void *init_states, const void *points, const void *scalars, void *ok, void *mega,
                            void *challenges_out, const uint8_t *gadget_label = nullptr, void *chi_out = nullptr) {
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  Words8 *chp;
  void *dbad, *dchi;
  CK(fs_transcript_locked(ctx, c, nb, k, init_states, points, scalars, challenges_out, gadget_label, chi_out, &chp, &dbad, &dchi));
  CK(verify_batch_dev_locked(ctx, g, c, nb, n1, k, points, scalars, chp, ok, mega, nullptr, dchi));
  and_not(ctx->st, (int32_t *)ok, (const int32_t *)dbad, nb);
  return launch_ok(ctx);
}
int bpgpu_r1cs_verify_batch_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                   const void *init_states, const void *points, const void *scalars, void *ok, void *mega,
                                   void *challenges_out) {
  if (!ctx || !g || !c || (nb && (!init_states || !points || !scalars || !ok))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_fs_locked(ctx, g, c, nb, n1, k, init_states, points, scalars, ok, mega, challenges_out);
}
// bpgpu_r1cs_verify_batch_fs(2) after their argument checks: the operands go up, the verdicts and challenges come back
static int verify_fs_host(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                          const uint8_t *init_states, const uint8_t *gadget_label, const uint8_t *points, const uint8_t *scalars,
                          int32_t *ok, uint8_t *mega, uint8_t *challenges_out, uint8_t *gadget_challenges_out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t nvar = verify_nvar(c, k);
  void *dP, *dS, *dI, *dok, *dmega, *dcho, *dchi;
  CK(ws_get(ctx, WS_ARG0, nb * nvar * 64, &dP));
  CK(ws_get(ctx, WS_ARG1, nb * 5 * 32, &dS));
  CK(ws_get(ctx, WS_ARG2, nb * 32, &dI));
  CK(ws_get(ctx, WS_ARG3, nb * 4 + nb * 64, &dok));
  dmega = (uint8_t *)dok + ((nb * 4 + 63) / 64) * 64;
  CK(ws_get(ctx, WS_FS_STAGE, nb * (6 + k) * 32, &dcho));
  CK(ws_get(ctx, WS_CHI_OUT, nb * (c->nchi ? c->nchi : 1) * 32, &dchi));
  CK(h2d(ctx, dP, points, nb * nvar * 64));
  CK(h2d(ctx, dS, scalars, nb * 5 * 32));
  CK(h2d(ctx, dI, init_states, nb * 32));
  CK(verify_fs_locked(ctx, g, c, nb, n1, k, dI, dP, dS, dok, mega ? dmega : nullptr, dcho, gadget_label, c->nchi ? dchi : nullptr));
  CK(d2h(ctx, ok, dok, nb * 4));
  if (mega) CK(d2h(ctx, mega, dmega, nb * 64));
  if (challenges_out) CK(d2h(ctx, challenges_out, dcho, nb * (6 + k) * 32));
  if (gadget_challenges_out && c->nchi) CK(d2h(ctx, gadget_challenges_out, dchi, nb * c->nchi * 32));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
int bpgpu_r1cs_verify_batch_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                               const uint8_t *init_states, const uint8_t *points, const uint8_t *scalars, int32_t *ok,
                               uint8_t *mega, uint8_t *challenges_out) {
  if (!ctx || !g || !c || (nb && (!init_states || !points || !scalars || !ok))) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  return verify_fs_host(ctx, g, c, nb, n1, k, init_states, nullptr, points, scalars, ok, mega, challenges_out, nullptr);
}

/* two-phase circuits (parametric constraint weights): host challenges + gadget challenges, or the transcript on the device */
int bpgpu_r1cs_verify_batch_param(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                  size_t k, const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges,
                                  const uint8_t *gadget_challenges, int32_t *ok, uint8_t *mega, uint8_t *msm_scalars) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !ok)) || (c && c->nchi && !gadget_challenges)) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  return verify_batch_host(ctx, g, c, nb, n1, k, points, scalars, challenges, gadget_challenges, ok, mega, msm_scalars);
}
int bpgpu_r1cs_verify_batch_fs2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                    const void *init_states, const uint8_t gadget_label[32], const void *points, const void *scalars,
                                    void *ok, void *mega, void *challenges_out, void *gadget_challenges_out) {
  if (!ctx || !g || !c || (nb && (!init_states || !points || !scalars || !ok))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_fs_locked(ctx, g, c, nb, n1, k, init_states, points, scalars, ok, mega, challenges_out, gadget_label, gadget_challenges_out);
}
int bpgpu_r1cs_verify_batch_fs2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *points,
                                const uint8_t *scalars, int32_t *ok, uint8_t *mega, uint8_t *challenges_out,
                                uint8_t *gadget_challenges_out) {
  if (!ctx || !g || !c || (nb && (!init_states || !points || !scalars || !ok))) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  return verify_fs_host(ctx, g, c, nb, n1, k, init_states, gadget_label, points, scalars, ok, mega, challenges_out, gadget_challenges_out);
}

/* ---------------------------------------------------------------- Verifier::verify from wire-format proofs */
// proof_len -> (two_phase, k): 1 + (11 | 14) * 32 + (2k + 2) * 32; the two families never share a length
static bool wire_dims(size_t proof_len, int *two_phase, size_t *k) {
  if (proof_len < 1 + 13 * 32 || (proof_len - 1) % 32) return false;
  size_t el = (proof_len - 1) / 32;
  if (el >= 13 && (el - 13) % 2 == 0) { *two_phase = 0; *k = (el - 13) / 2; return *k < 32; }
  if (el >= 16 && (el - 16) % 2 == 0) { *two_phase = 1; *k = (el - 16) / 2; return *k < 32; }
  return false;
}
// the context's square-root tables, built on its stream at first use
static int sqrt_tab_locked(bpgpu_ctx *ctx) {
  if (ctx->sqrt_tab) return BPGPU_OK;
  void *t = nullptr;
  if (hipMalloc(&t, sqrt_table_bytes()) != hipSuccess) return BPGPU_E_OOM;
  sqrt_tables_build(ctx->st, t);
  ctx->sqrt_tab = t;
  return BPGPU_OK;
}
// sqrt_tab: tables another context owns and has built before this one's stream forked from it (a lane of a mixed wire call);
// null: the context's own
static int verify_wire_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                              size_t proof_len, const void *proofs, const void *commitments, const void *init_states,
                              void *ok, const uint8_t *gadget_label = nullptr, const void *sqrt_tab = nullptr) {
  int two_phase = 0;
  size_t k = 0;
  if (!wire_dims(proof_len, &two_phase, &k)) return BPGPU_E_LEN;
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (!sqrt_tab) { CK(sqrt_tab_locked(ctx)); sqrt_tab = ctx->sqrt_tab; }
  const size_t m = c->m, nvar = verify_nvar(c, k);
  void *dcomp, *dxy, *dsc, *dfmt;
  CK(ws_get(ctx, WS_ARG0, nb * nvar * 32, &dcomp));
  CK(ws_get(ctx, WS_ARG1, nb * nvar * 64, &dxy));
  CK(ws_get(ctx, WS_ARG2, nb * 5 * 32, &dsc));
  CK(ws_get(ctx, WS_VAUX, nb * 4 + nb * nvar * 4, &dfmt));
  int32_t *fmt_ok = (int32_t *)dfmt, *dec_ok = fmt_ok + nb;
  wire_unpack(ctx->st, (const uint8_t *)proofs, proof_len, (const uint8_t *)commitments, nb, m, k, two_phase,
              (Words8 *)dcomp, (Words8 *)dsc, fmt_ok);
  points_decompress(ctx->st, (const Words8 *)dcomp, (Words8 *)dxy, dec_ok, nb * nvar, sqrt_tab);
  // undecodable points come out as the identity: the transcript / MSM run on them, the verdict is forced to 0 below
  CK(verify_fs_locked(ctx, g, c, nb, n1, k, init_states, dxy, dsc, ok, nullptr, nullptr, gadget_label));
  wire_and_ok(ctx->st, (int32_t *)ok, fmt_ok, dec_ok, nb, nvar);
  return launch_ok(ctx);
}
// (gadget_label: null for the entry points without one -- a parametric circuit is then refused by the transcript half)
static int verify_wire_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t proof_len,
                           const uint8_t *gadget_label, const void *proofs_dev, const void *commitments_dev, const void *init_states_dev,
                           void *ok_dev) {
  if (!ctx || !g || !c || (nb && (!proofs_dev || !init_states_dev || !ok_dev || (c->m && !commitments_dev)))) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_wire_locked(ctx, g, c, nb, n1, proof_len, proofs_dev, commitments_dev, init_states_dev, ok_dev, gadget_label);
}
int bpgpu_r1cs_verify_batch_wire_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                     size_t proof_len, const void *proofs_dev, const void *commitments_dev,
                                     const void *init_states_dev, void *ok_dev) {
  return verify_wire_dev(ctx, g, c, nb, n1, proof_len, nullptr, proofs_dev, commitments_dev, init_states_dev, ok_dev);
}
int bpgpu_r1cs_verify_batch_wire2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                      size_t proof_len, const uint8_t gadget_label[32], const void *proofs_dev,
                                      const void *commitments_dev, const void *init_states_dev, void *ok_dev) {
  if (!gadget_label && !(c && circuit_labels(c))) return BPGPU_E_ARG;   // the label: the call's, or the circuit's own
  return verify_wire_dev(ctx, g, c, nb, n1, proof_len, gadget_label, proofs_dev, commitments_dev, init_states_dev, ok_dev);
}
static int verify_wire_host(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t proof_len,
                            const uint8_t *gadget_label, const uint8_t *proofs, const uint8_t *commitments, const uint8_t *init_states,
                            int32_t *ok) {
  if (!ctx || !g || !c || (nb && (!proofs || !init_states || !ok || (c->m && !commitments)))) return BPGPU_E_ARG;
  if (!nb) return BPGPU_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t m = c->m;
  void *dP, *dC, *dI, *dok;
  CK(ws_get(ctx, WS_ARG3, nb * proof_len + 64, &dP));
  CK(ws_get(ctx, WS_ARG4, nb * (m ? m : 1) * 32, &dC));
  CK(ws_get(ctx, WS_ARG5, nb * 32, &dI));
  CK(ws_get(ctx, WS_FS_STAGE, nb * 4, &dok));
  CK(h2d(ctx, dP, proofs, nb * proof_len));
  if (m) CK(h2d(ctx, dC, commitments, nb * m * 32));
  CK(h2d(ctx, dI, init_states, nb * 32));
  CK(verify_wire_locked(ctx, g, c, nb, n1, proof_len, dP, dC, dI, dok, gadget_label));
  CK(d2h(ctx, ok, dok, nb * 4));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}
int bpgpu_r1cs_verify_batch_wire(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                 size_t proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                 const uint8_t *init_states, int32_t *ok) {
  return verify_wire_host(ctx, g, c, nb, n1, proof_len, nullptr, proofs, commitments, init_states, ok);
}
int bpgpu_r1cs_verify_batch_wire2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                  size_t proof_len, const uint8_t gadget_label[32], const uint8_t *proofs, const uint8_t *commitments,
                                  const uint8_t *init_states, int32_t *ok) {
  if (!gadget_label && !(c && circuit_labels(c))) return BPGPU_E_ARG;   // the label: the call's, or the circuit's own
  return verify_wire_host(ctx, g, c, nb, n1, proof_len, gadget_label, proofs, commitments, init_states, ok);
}

/* ---------------------------------------------------------------- combined batch check
 * sum_p rho_p * mega_check_p as ONE point: the generator terms collapse to a single fixed-base MSM with
 * scalars sum_p rho_p * s_{p,g}; the proof-specific points go through one bucket-method MSM of
 * nb * (11 + m + 2k) terms.  All proofs are valid iff the (all-GPU) sum of the partial points is the
 * identity, up to the 2^-252 soundness of the random weights.  Not a reference API: offered
 * beside the per-proof mode for verifier services; the per-proof mode stays the parity path. */
static int verify_combined_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                  size_t k, const void *points, const void *scalars, const void *challenges,
                                  const void *rho, void *partial_xy) {
  if (k >= 32) return BPGPU_E_LEN;
  CK(verify_shape(c, g, n1, k));
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)1 << k, nvar = verify_nvar(c, k), nfix = 2 + 2 * np, tot = nb * nvar;
  void *dpts, *dfix, *dvar, *dzp, *dfsum, *dtwo, *dsum, *dpip;
  CK(ws_get(ctx, WS_VPTS, tot * sizeof(AffDev), &dpts));
  CK(ws_get(ctx, WS_VFIX, nb * nfix * 32, &dfix));
  CK(ws_get(ctx, WS_VVAR, tot * 32, &dvar));
  if (c->nchi) return BPGPU_E_ARG;
  VerifyDims d{nb, n1, c->n, np, k, c->m, nullptr, (size_t)ctx->opt[BPGPU_OPT_VS_LARGE_MIN]};
  CK(ws_get(ctx, WS_ZPOW, verify_scalars_scratch_ints(circuit_dev(c), d) * 4, &dzp));
  CK(ws_get(ctx, WS_VVRES, nfix * 32, &dfsum));
  CK(ws_get(ctx, WS_VFRES, 2 * sizeof(JacRaw), &dtwo));
  CK(ws_get(ctx, WS_VAUX, sizeof(JacRaw), &dsum));
  CK(flag_reset(ctx));
  if (verify_combined2_supported(nb, nvar, g->c, np)) {   // eight launches on one stream (k_pip2.hip)
    void *dc2;
    CK(ws_get(ctx, WS_PIP, verify_combined2_scratch_bytes(nb, nvar, nfix), &dc2));
    CombinedArgs ca{circuit_dev(c), d, nvar, (const Words8 *)points, (const Words8 *)scalars, (const Words8 *)challenges,
                    (const Words8 *)rho, (Words8 *)dfix, (Words8 *)dvar, (int32_t *)dzp, g->table, g->cap, g->c, dc2, ctx->d_flag,
                    (Words8 *)partial_xy, ctx->prof ? &prof_mark_cb : nullptr, ctx};
    verify_combined2(ctx->st, ca);
    return launch_ok(ctx);
  }
  const int cw = pippenger_window(tot);
  CK(ws_get(ctx, WS_PIP, pippenger_scratch_bytes(tot, cw), &dpip));
  // (canonicity of the scalars and challenges is checked inside verify_scalars)
  scalars_check(ctx->st, (const Words8 *)rho, nb, ctx->d_flag);
  verify_scalars(ctx->st, circuit_dev(c), d, (const Words8 *)challenges, (const Words8 *)scalars, (Words8 *)dfix,
                 (Words8 *)dvar, nullptr, (int32_t *)dzp, ctx->d_flag);
  // generator part on stream 2: weighted column sums, then one fixed-base MSM
  CK(side_fork(ctx));
  sc_weighted_colsum(ctx->st2, nb, nfix, (const Words8 *)dfix, (const Words8 *)rho, (Words8 *)dfsum);
  CK(msm_gens_dev(ctx, g, 1, np, (const uint32_t *)dfsum, (JacRaw *)dtwo, ctx->st2));
  CK(side_done(ctx));
  // proof-specific points on stream 1: scale by rho, bucket-method MSM
  points_from_boundary(ctx->st, (const Words8 *)points, (AffDev *)dpts, tot, ctx->d_flag);
  sc_scale_rows(ctx->st, nb, nvar, (Words8 *)dvar, (const Words8 *)rho);
  pippenger(ctx->st, (const AffDev *)dpts, (const uint32_t *)dvar, tot, cw, (JacRaw *)dtwo + 1, dpip);
  CK(side_join(ctx));
  segmented_sum(ctx->st, (const JacRaw *)dtwo, (JacRaw *)dsum, 1, 2);
  jac_to_boundary(ctx->st, (const JacRaw *)dsum, (Words8 *)partial_xy, 1);
  return launch_ok(ctx);
}
int bpgpu_r1cs_verify_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                   size_t k, const void *points, const void *scalars, const void *challenges,
                                   const void *rho, void *partial_xy_dev) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !rho)) || !partial_xy_dev) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_combined_locked(ctx, g, c, nb, n1, k, points, scalars, challenges, rho, partial_xy_dev);
}
int bpgpu_r1cs_verify_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                               size_t k, const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges,
                               const uint8_t *rho, uint8_t partial_xy[64]) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !rho)) || !partial_xy) return BPGPU_E_ARG;
  if (k >= 32) return BPGPU_E_LEN;
  if (!nb) { memset(partial_xy, 0, 64); return BPGPU_OK; }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t nvar = verify_nvar(c, k);
  void *dP, *dS, *dC, *dR, *dout;
  CK(ws_get(ctx, WS_ARG0, nb * nvar * 64, &dP));
  CK(ws_get(ctx, WS_ARG1, nb * 5 * 32, &dS));
  CK(ws_get(ctx, WS_ARG2, nb * (6 + k) * 32, &dC));
  CK(ws_get(ctx, WS_ARG3, nb * 32, &dR));
  CK(ws_get(ctx, WS_ARG4, 64, &dout));
  CK(h2d(ctx, dP, points, nb * nvar * 64));
  CK(h2d(ctx, dS, scalars, nb * 5 * 32));
  CK(h2d(ctx, dC, challenges, nb * (6 + k) * 32));
  CK(h2d(ctx, dR, rho, nb * 32));
  CK(verify_combined_locked(ctx, g, c, nb, n1, k, dP, dS, dC, dR, dout));
  int bad = 0;
  CK(flag_read(ctx, &bad));
  if (bad) return BPGPU_E_ARG;
  CK(d2h(ctx, partial_xy, dout, 64));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}

/* The two phases of a screened call over `nchecks` checks, each forked over the lanes and joined.  Phase 1: check(ln, ci, partial) on
 * lane ci % nl writes check ci's point to `partial` (HBM) and leaves its malformed-input flag in ln->d_flag, which is copied beside
 * it; the host reads every point and flag at once.  Phase 2: a check passes when its flag is 0 and its point is the identity (64
 * zero bytes): accept(ci) marks its proofs valid; the others go to fallback(ln, ci), round-robin over the lanes. */
extern "C++" {   // (a template, in the middle of the C ABI)
template <class Check, class Accept, class Fallback>
static int screen_locked(bpgpu_ctx *ctx, size_t nchecks, const char *what, size_t *fallback_batches, Check check, Accept accept,
                         Fallback fallback) try {
  const size_t nlanes_opt = (size_t)ctx->opt[BPGPU_OPT_STREAM_LANES], nl = nchecks < nlanes_opt ? nchecks : nlanes_opt;
  CK(stream_lanes(ctx, nl));
  void *dpart, *dflag;
  CK(ws_get(ctx, WS_SCREEN_PART, nchecks * 64, &dpart));
  CK(ws_get(ctx, WS_SCREEN_FLAG, nchecks * 4, &dflag));
  std::vector<uint8_t> hpart(nchecks * 64);
  std::vector<int> hflag(nchecks);
  CK(lanes_fork(ctx, nl));
  int rc = BPGPU_OK;
  for (size_t ci = 0; ci < nchecks && rc == BPGPU_OK; ci++) {
    bpgpu_ctx *ln = ctx->lanes[ci % nl];
    rc = check(ln, ci, (uint8_t *)dpart + 64 * ci);
    if (rc == BPGPU_OK && hipMemcpyAsync((int *)dflag + ci, ln->d_flag, 4, hipMemcpyDeviceToDevice, ln->st) != hipSuccess) rc = BPGPU_E_DEVICE;
    if (rc) ctx->err = ln->err;
  }
  CK(lanes_join(ctx, nl, rc, what));
  CK(d2h(ctx, hpart.data(), dpart, nchecks * 64));
  CK(d2h(ctx, hflag.data(), dflag, nchecks * 4));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  size_t nfall = 0;
  CK(lanes_fork(ctx, nl));
  for (size_t ci = 0; ci < nchecks && rc == BPGPU_OK; ci++) {
    bool pass = hflag[ci] == 0;
    for (size_t i = 0; i < 64 && pass; i++) pass = hpart[64 * ci + i] == 0;
    if (pass) { rc = accept(ci); continue; }
    bpgpu_ctx *ln = ctx->lanes[nfall++ % nl];
    rc = fallback(ln, ci);
    if (rc) ctx->err = ln->err;
  }
  rc = lanes_join(ctx, nl, rc, what);
  if (fallback_batches) *fallback_batches = nfall;
  return rc;
} catch (const std::bad_alloc &) {
  return BPGPU_E_OOM;
}
}  // extern "C++"

/* Screened stream: the combined check of every batch first (one point per batch), the per-proof path only for the batches whose
 * point is not the identity (or that hold a malformed input). */
// init_states != null: the transcript is replayed on the device (challenges unused): per batch k_verify_transcript first, and a proof
// whose transcript replay fails (a validated point is the identity) sends its batch to the per-proof path like any other failure
static int verify_screened_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                  const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho,
                                  uint8_t *ok, bool on_host, size_t *fallback_batches, const uint8_t *init_states = nullptr) {
  if (k >= 32) return BPGPU_E_LEN;
  if (fallback_batches) *fallback_batches = 0;
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  // proofs per combined check: the check is a chain of nine mostly latency-bound launches with little work per proof, so its
  // batches are larger than the per-proof path's (2560 x 24 points still fit the one-instance bucket pipeline of k_pip2.hip:
  // 11.2 M/s against 8.1 M/s at 1024); a batch that fails is re-verified proof by proof as a whole
  const size_t nvar = verify_nvar(c, k), nch = 6 + k;
  size_t batch = (size_t)ctx->opt[BPGPU_OPT_SCREEN_BATCH];
  const size_t fit = ((size_t)1 << 16) / nvar / 64 * 64;          // proof points of one check <= 2^16
  if (fit >= 256 && batch > fit) batch = fit;
  const size_t nchunks = (nb + batch - 1) / batch;
  auto count = [&](size_t lo) { return nb - lo < batch ? nb - lo : batch; };
  // stage a batch's operands on its lane (host variant); returns device pointers either way
  // (*Cc = the challenges, or with a device transcript the batch's 32-byte initial states)
  const uint8_t *third = init_states ? init_states : challenges;
  const size_t third_bytes = init_states ? 32 : nch * 32;
  auto operands = [&](bpgpu_ctx *ln, size_t lo, size_t cnt, const void **P, const void **S, const void **Cc, const void **R, void **dok) -> int {
    if (!on_host) {
      *P = points + lo * nvar * 64; *S = scalars + lo * 5 * 32; *Cc = third + lo * third_bytes; *R = rho + lo * 32; *dok = ok + lo * 4;
      return BPGPU_OK;
    }
    void *dP, *dS, *dC, *dR;
    int rc;
    if ((rc = ws_get(ln, WS_ARG0, batch * nvar * 64, &dP)) || (rc = ws_get(ln, WS_ARG1, batch * 5 * 32, &dS)) || (rc = ws_get(ln, WS_ARG2, batch * third_bytes, &dC)) ||
        (rc = ws_get(ln, WS_ARG3, batch * 32, &dR)) || (rc = ws_get(ln, WS_ARG4, batch * 4, dok)) ||
        (rc = h2d(ln, dP, points + lo * nvar * 64, cnt * nvar * 64)) || (rc = h2d(ln, dS, scalars + lo * 5 * 32, cnt * 5 * 32)) ||
        (rc = h2d(ln, dC, third + lo * third_bytes, cnt * third_bytes)) || (rc = h2d(ln, dR, rho + lo * 32, cnt * 32)))
      return rc;
    *P = dP; *S = dS; *Cc = dC; *R = dR;
    return BPGPU_OK;
  };
  auto check = [&](bpgpu_ctx *ln, size_t ci, void *partial) -> int {
    const size_t lo = ci * batch, cnt = count(lo);
    const void *P, *S, *Cc, *R;
    void *dok, *dbad = nullptr, *dchi = nullptr;
    CK(operands(ln, lo, cnt, &P, &S, &Cc, &R, &dok));
    if (init_states) {       // the batch's challenges from the device transcript
      Words8 *chp = nullptr;
      CK(fs_transcript_locked(ln, c, cnt, k, Cc, P, S, nullptr, nullptr, nullptr, &chp, &dbad, &dchi));
      Cc = chp;
    }
    CK(verify_combined_locked(ln, g, c, cnt, n1, k, P, S, Cc, R, partial));
    if (dbad) or_flag(ln->st, (const int32_t *)dbad, cnt, ln->d_flag);      // (after the combined check: it resets the flag)
    zero_flag(ln->st, (const Words8 *)R, cnt, ln->d_flag);                   // a zero weight voids the check for its batch
    return BPGPU_OK;
  };
  auto accept = [&](size_t ci) -> int {
    const size_t lo = ci * batch, cnt = count(lo);
    if (on_host) for (size_t i = 0; i < cnt; i++) ((int32_t *)ok)[lo + i] = 1;
    else if (hipMemsetD32Async((hipDeviceptr_t)(ok + lo * 4), 1, cnt, ctx->st) != hipSuccess) return BPGPU_E_DEVICE;
    return BPGPU_OK;
  };
  auto fallback = [&](bpgpu_ctx *ln, size_t ci) -> int {
    const size_t lo = ci * batch, cnt = count(lo);
    const void *P, *S, *Cc, *R;
    void *dok;
    CK(operands(ln, lo, cnt, &P, &S, &Cc, &R, &dok));
    CK(init_states ? verify_fs_locked(ln, g, c, cnt, n1, k, Cc, P, S, dok, nullptr, nullptr)
                   : verify_batch_dev_locked(ln, g, c, cnt, n1, k, P, S, Cc, dok, nullptr, nullptr));
    return on_host ? d2h(ln, ok + lo * 4, dok, cnt * 4) : BPGPU_OK;
  };
  return screen_locked(ctx, nchunks, "bpgpu_r1cs_verify_screened", fallback_batches, check, accept, fallback);
}
int bpgpu_r1cs_verify_screened_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                      const void *init_states_dev, const void *points_dev, const void *scalars_dev, const void *rho_dev,
                                      void *ok_dev, size_t *fallback_batches) {
  if (!ctx || !g || !c || (nb && (!init_states_dev || !points_dev || !scalars_dev || !rho_dev || !ok_dev))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_screened_locked(ctx, g, c, nb, n1, k, (const uint8_t *)points_dev, (const uint8_t *)scalars_dev, nullptr,
                                (const uint8_t *)rho_dev, (uint8_t *)ok_dev, false, fallback_batches, (const uint8_t *)init_states_dev);
}
int bpgpu_r1cs_verify_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                   const void *points_dev, const void *scalars_dev, const void *challenges_dev, const void *rho_dev,
                                   void *ok_dev, size_t *fallback_batches) {
  if (!ctx || !g || !c || (nb && (!points_dev || !scalars_dev || !challenges_dev || !rho_dev || !ok_dev))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_screened_locked(ctx, g, c, nb, n1, k, (const uint8_t *)points_dev, (const uint8_t *)scalars_dev,
                                (const uint8_t *)challenges_dev, (const uint8_t *)rho_dev, (uint8_t *)ok_dev, false, fallback_batches);
}
int bpgpu_r1cs_verify_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                               const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, int32_t *ok,
                               size_t *fallback_batches) {
  if (!ctx || !g || !c || (nb && (!points || !scalars || !challenges || !rho || !ok))) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (fallback_batches) *fallback_batches = 0;
  if (!nb) return BPGPU_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  CK(pinned_verdicts(ctx, nb));
  CK(verify_screened_locked(ctx, g, c, nb, n1, k, points, scalars, challenges, rho, (uint8_t *)ctx->pinned, true, fallback_batches));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  memcpy(ok, ctx->pinned, nb * 4);
  return BPGPU_OK;
}

/* ---------------------------------------------------------------- mixed queues: proofs of several circuits in one call
 * The groups' proofs are concatenated (group after group) and cut into checks; a check is a list of runs ("segments") of one group's
 * consecutive proofs (queue_plan.h: mixed_plan, host arithmetic with a CPU test of its own).  Each check is ONE ragged combined check
 * (k_mixed.hip); the screened call re-verifies a failing check per proof, segment by segment, on each segment's own circuit.
 * A queue holds decoded operands (bpgpu_verify_group) or wire bytes (bpgpu_wire_group).  The plan, the two drivers, the host staging
 * and the entry helpers are stated once, over a queue kind (DecodedQueue, WireQueue) that says what differs:
 *   validate(screened)                 shape checks of every group before anything is launched (the codes of the one-circuit calls;
 *                                      screened: ok[] must be given); leaves what the plan reads in shape[]
 *   prepare(ctx)                       once per call on the calling context, when the plan is not empty and before any lane forks
 *   front(ln, segs, nseg, bit, in)     the segment table of ONE check on lane ln; what it launches ORs `bit` into ln's input flag
 *   per_proof(ln, seg)                 the per-proof path of one segment on lane ln: verdicts into the group's ok[] (HBM)
 *   fields(x, d, f)                    host forms: the operand fields of group x, and where their device addresses go in its copy d */
using bpqueue::MixCheck;
using bpqueue::MixSeg;
using bpqueue::QueueShape;
namespace {
struct StageField { const void *src; const void **dst; size_t bytes; };
}
// a segment's entry of a check's table: cnt proofs of circuit c from the given operands
static MixSegIn mixed_seg_in(const bpgpu_ctx *ln, const bpgpu_circuit *c, size_t cnt, size_t n1, size_t k, const Words8 *points,
                             const Words8 *proof_scalars, const Words8 *challenges, const Words8 *chi, const Words8 *rho) {
  MixSegIn v;
  v.circ = circuit_dev(c);
  v.d = VerifyDims{cnt, n1, c->n, (size_t)1 << k, k, c->m, c->nchi ? chi : nullptr, (size_t)ln->opt[BPGPU_OPT_VS_LARGE_MIN]};
  v.nvar = verify_nvar(c, k); v.nchi = c->nchi;
  v.points = points; v.proof_scalars = proof_scalars; v.challenges = challenges;
  v.rho = rho;
  return v;
}
// ONE ragged combined check on `ln`'s stream: partial_xy (HBM) = sum over the check's proofs of rho_p * mega_check_p.  The caller
// resets ln's input flag; zero_rho (optional) is raised for a zero weight.
static int mixed_run_locked(bpgpu_ctx *ln, const bpgpu_gens *g, const MixSegIn *in, size_t nseg, void *partial_xy, int *zero_rho) {
  void *scr;
  CK(ws_get(ln, WS_PIP, verify_mixed_scratch_bytes(in, nseg, g->c), &scr));
  MixedArgs a{in, nseg, scr, g->table, g->cap, g->c, ln->d_flag, zero_rho, (Words8 *)partial_xy, ln->prof ? &prof_mark_cb : nullptr, ln};
  verify_mixed(ln->st, a);
  return launch_ok(ln);
}

/* ---- decoded operands (bpgpu_r1cs_verify_mixed_*): the front is pointer arithmetic on the groups' arrays ---- */
// the per-proof path for one segment on lane ln: bpgpu_r1cs_verify_batch(_param)'s verdicts into the group's ok[] (HBM)
static int mixed_per_proof_locked(bpgpu_ctx *ln, const bpgpu_gens *g, const bpgpu_verify_group &x, size_t lo, size_t cnt) {
  const bpgpu_circuit *c = x.circuit;
  const size_t nvar = verify_nvar(x.circuit, x.k);
  const Words8 *chi = c->nchi ? (const Words8 *)x.gadget_challenges + lo * c->nchi : nullptr;
  int32_t *ok = (int32_t *)x.ok + lo;
  void *dchibad = nullptr;
  if (chi) {        // a non-canonical gadget challenge rejects ITS proof, as in bpgpu_r1cs_verify_batch_param
    CK(ws_get(ln, WS_PROOF_BAD, cnt * 4, &dchibad));
    HIPCK(ln, hipMemsetAsync(dchibad, 0, cnt * 4, ln->st));
    scalars_check_proof(ln->st, chi, cnt * c->nchi, c->nchi, ln->d_flag, (int32_t *)dchibad);
  }
  CK(verify_batch_dev_locked(ln, g, c, cnt, x.n1, x.k, (const uint8_t *)x.points + lo * nvar * 64, (const uint8_t *)x.scalars + lo * 160,
                             (const uint8_t *)x.challenges + lo * (6 + x.k) * 32, ok, nullptr, nullptr, chi));
  if (dchibad) and_not(ln->st, ok, (const int32_t *)dchibad, cnt);
  return launch_ok(ln);
}
namespace {
struct DecodedQueue {
  using Group = bpgpu_verify_group;
  static constexpr const char *screened_name = "bpgpu_r1cs_verify_mixed_screened";
  static constexpr size_t NFIELDS = 5;
  const bpgpu_gens *g;
  const Group *G;
  size_t ngroups;
  QueueShape shape[BPGPU_MIXED_MAX_GROUPS];
  int validate(bool screened) {
    if (!g || (ngroups && !G) || ngroups > BPGPU_MIXED_MAX_GROUPS) return BPGPU_E_ARG;
    for (size_t i = 0; i < ngroups; i++) {
      const Group &x = G[i];
      const bpgpu_circuit *c = x.circuit;
      if (!c) return BPGPU_E_ARG;
      if (x.nb && (!x.points || !x.scalars || !x.challenges || !x.rho || (screened && !x.ok))) return BPGPU_E_ARG;
      if ((c->nchi != 0) != (x.gadget_challenges != nullptr)) return BPGPU_E_ARG;
      if (x.k >= 32) return BPGPU_E_LEN;
      CK(verify_shape(c, g, x.n1, x.k));
      shape[i] = QueueShape{x.nb, verify_nvar(c, x.k)};
    }
    return BPGPU_OK;
  }
  int prepare(bpgpu_ctx *) { return BPGPU_OK; }
  int front(bpgpu_ctx *ln, const MixSeg *segs, size_t nseg, int, MixSegIn *in) const {
    for (size_t s = 0; s < nseg; s++) {
      const Group &x = G[segs[s].gi];
      const size_t lo = segs[s].lo, nvar = shape[segs[s].gi].nvar;
      in[s] = mixed_seg_in(ln, x.circuit, segs[s].cnt, x.n1, x.k, (const Words8 *)x.points + lo * nvar * 2, (const Words8 *)x.scalars + lo * 5,
                           (const Words8 *)x.challenges + lo * (6 + x.k), (const Words8 *)x.gadget_challenges + lo * x.circuit->nchi,
                           (const Words8 *)x.rho + lo);
    }
    return BPGPU_OK;
  }
  int per_proof(bpgpu_ctx *ln, const MixSeg &sg) const { return mixed_per_proof_locked(ln, g, G[sg.gi], sg.lo, sg.cnt); }
  static void fields(const Group &x, Group &d, StageField *f) {
    f[0] = StageField{x.points, &d.points, x.nb * verify_nvar(x.circuit, x.k) * 64};
    f[1] = StageField{x.scalars, &d.scalars, x.nb * 160};
    f[2] = StageField{x.challenges, &d.challenges, x.nb * (6 + x.k) * 32};
    f[3] = StageField{x.gadget_challenges, &d.gadget_challenges, x.gadget_challenges ? x.nb * x.circuit->nchi * 32 : 0};
    f[4] = StageField{x.rho, &d.rho, x.nb * 32};
  }
};
}

/* ---- WIRE-format proofs, transcript on the device (bpgpu_r1cs_verify_mixed_wire_*) ----
 * Per check a ragged front decodes the segments into the lane's workspace in four launches -- unpack, ONE decompression over the
 * check's points, the transcript replay, a fold of the reject bits -- in the layouts of MixSegIn, and the ragged combined check runs
 * on them unchanged.  The square-root tables and the groups' transcript schedules are built / uploaded once per call on the calling
 * context, before the lanes fork; the lanes only read them. */
namespace {
struct WireGroupDims { int two_phase; size_t k; };
struct WireSched { const TrStep *steps; int nsteps; const uint8_t *labels; };   // labels: the circuit's label table in HBM, or null
}
// every non-empty group's schedule (and behind it the label table of a circuit that has one), one after the other in WS_WIRE_SCHED of
// the calling context: ONE upload per call from page-locked staging, no host wait (fs_transcript_locked's one-entry cache would re-upload and wait whenever the shape changes)
static int wire_schedules_locked(bpgpu_ctx *ctx, const bpgpu_wire_group *G, const WireGroupDims *dims, size_t ngroups, WireSched *out) {
  size_t cap = 0;
  auto room = [&](size_t i) { return transcript_schedule_max(G[i].circuit->m, dims[i].k, G[i].circuit->nchi) + gadget_label_slots(G[i].circuit->nchi); };
  for (size_t i = 0; i < ngroups; i++) if (G[i].nb) cap += room(i);
  if (!cap) return BPGPU_OK;
  if (!ctx->wsched_ev) HIPCK(ctx, hipEventCreateWithFlags(&ctx->wsched_ev, hipEventDisableTiming));
  else HIPCK(ctx, hipEventSynchronize(ctx->wsched_ev));        // the previous call's upload has read the staging
  if (ctx->wsched_cap < cap * sizeof(TrStep)) {
    if (ctx->wsched_host) { (void)hipHostFree(ctx->wsched_host); ctx->wsched_host = nullptr; ctx->wsched_cap = 0; }
    HIPCK(ctx, hipHostMalloc(&ctx->wsched_host, 2 * cap * sizeof(TrStep), hipHostMallocDefault));
    ctx->wsched_cap = 2 * cap * sizeof(TrStep);
  }
  void *dsteps;
  CK(ws_get(ctx, WS_WIRE_SCHED, cap * sizeof(TrStep), &dsteps));
  TrStep *h = (TrStep *)ctx->wsched_host;
  size_t off = 0;
  for (size_t i = 0; i < ngroups; i++) {
    if (!G[i].nb) { out[i] = WireSched{nullptr, 0, nullptr}; continue; }
    const bpgpu_circuit *c = G[i].circuit;
    memset(h + off, 0, room(i) * sizeof(TrStep));
    const int n = transcript_schedule(h + off, c->m, dims[i].k, (size_t)1 << dims[i].k, c->nchi);
    out[i] = WireSched{(const TrStep *)dsteps + off, n, nullptr};
    off += (size_t)n;
    if (const uint8_t *labels = circuit_labels(c)) {
      memcpy(h + off, labels, c->nchi * GADGET_LABEL_BYTES);
      out[i].labels = (const uint8_t *)((const TrStep *)dsteps + off);
      off += gadget_label_slots(c->nchi);
    }
  }
  HIPCK(ctx, hipMemcpyAsync(dsteps, h, off * sizeof(TrStep), hipMemcpyHostToDevice, ctx->st));
  HIPCK(ctx, hipEventRecord(ctx->wsched_ev, ctx->st));
  return BPGPU_OK;
}
// The ragged front of ONE check on `ln`'s stream: fills in[] with the decoded operands (in ln's workspace) and ORs `bit` into ln's
// input flag when a proof of the check does not decode or fails the transcript's point validation.  The caller has reset the flag.
static int wire_front_locked(bpgpu_ctx *ln, const bpgpu_wire_group *G, const WireGroupDims *dims, const WireSched *sched,
                             const void *sqrt_tab, const MixSeg *segs, size_t nseg, int bit, MixSegIn *in) {
  size_t tot = 0, nbt = 0, nchs = 0, nchis = 0;
  for (size_t s = 0; s < nseg; s++) {
    const size_t gi = segs[s].gi;
    nchis += segs[s].cnt * G[gi].circuit->nchi;
    tot += segs[s].cnt * verify_nvar(G[gi].circuit, dims[gi].k);
    nbt += segs[s].cnt;
    nchs += segs[s].cnt * (6 + dims[gi].k);
  }
  if (tot + 5 * nbt >= ((size_t)1 << 31)) return BPGPU_E_LEN;      // (the front's tables index with 32 bits)
  void *dcomp, *dxy, *dsc, *dch, *dchi, *dbits, *dbad;
  CK(ws_get(ln, WS_ARG0, tot * 32, &dcomp));
  CK(ws_get(ln, WS_ARG1, tot * 64, &dxy));
  CK(ws_get(ln, WS_ARG2, nbt * 5 * 32, &dsc));
  CK(ws_get(ln, WS_FS_CH, nchs * 32, &dch));
  CK(ws_get(ln, WS_CHI, (nchis ? nchis : 1) * 32, &dchi));
  CK(ws_get(ln, WS_VAUX, (2 * nbt + tot) * 4, &dbits));
  CK(ws_get(ln, WS_PROOF_BAD, nbt * 4, &dbad));
  int32_t *fmt_ok = (int32_t *)dbits, *tr_bad = fmt_ok + nbt, *dec_ok = tr_bad + nbt;
  WireSegIn ws[BPGPU_MIXED_MAX_SEGMENTS];
  TrSegIn ts[BPGPU_MIXED_MAX_SEGMENTS];
  size_t pt_off = 0, p_off = 0, ch_off = 0, chi_off = 0;
  for (size_t s = 0; s < nseg; s++) {
    const size_t gi = segs[s].gi, lo = segs[s].lo, cnt = segs[s].cnt, k = dims[gi].k;
    const bpgpu_wire_group &x = G[gi];
    const bpgpu_circuit *c = x.circuit;
    const size_t m = c->m, nvar = verify_nvar(c, k);
    ws[s] = WireSegIn{(const uint8_t *)x.proofs + lo * x.proof_len, m ? (const uint8_t *)x.commitments + lo * m * 32 : nullptr, x.proof_len,
                      cnt, m, k, dims[gi].two_phase != 0};
    Words8 *pts = (Words8 *)dxy + pt_off * 2, *sc = (Words8 *)dsc + p_off * 5, *ch = (Words8 *)dch + ch_off, *chi = (Words8 *)dchi + chi_off;
    ts[s] = TrSegIn{sched[gi].steps, sched[gi].nsteps, cnt, m, k, c->nchi, (const Words8 *)x.init_states + lo, pts, sc, ch, chi,
                    tr_bad + p_off, x.gadget_label, sched[gi].labels};
    in[s] = mixed_seg_in(ln, c, cnt, x.n1, k, pts, sc, ch, chi, (const Words8 *)x.rho + lo);
    pt_off += cnt * nvar; p_off += cnt; ch_off += cnt * (6 + k); chi_off += cnt * c->nchi;
  }
  { ProfScope ps(ln, 23, ln->st);
    wire_unpack_ragged(ln->st, ws, nseg, (Words8 *)dcomp, (Words8 *)dsc, fmt_ok);
    // undecodable points come out as the identity: the transcript and the MSMs run on them, the fold rejects their proofs
    points_decompress(ln->st, (const Words8 *)dcomp, (Words8 *)dxy, dec_ok, tot, sqrt_tab); }
  { ProfScope ps(ln, 5, ln->st);
    verify_transcript_ragged(ln->st, ts, nseg); }
  { ProfScope ps(ln, 23, ln->st);
    wire_fold(ln->st, ws, nseg, fmt_ok, dec_ok, tr_bad, (int32_t *)dbad, ln->d_flag, bit); }
  return launch_ok(ln);
}
namespace {
struct WireQueue {
  using Group = bpgpu_wire_group;
  static constexpr const char *screened_name = "bpgpu_r1cs_verify_mixed_wire_screened";
  static constexpr size_t NFIELDS = 4;
  const bpgpu_gens *g;
  const Group *G;
  size_t ngroups;
  QueueShape shape[BPGPU_MIXED_MAX_GROUPS];
  WireGroupDims dims[BPGPU_MIXED_MAX_GROUPS];
  WireSched sched[BPGPU_MIXED_MAX_GROUPS];
  const void *sqrt_tab;                      // the calling context's
  int validate(bool screened) {
    if (!g || (ngroups && !G) || ngroups > BPGPU_MIXED_MAX_GROUPS) return BPGPU_E_ARG;
    for (size_t i = 0; i < ngroups; i++) {
      const Group &x = G[i];
      const bpgpu_circuit *c = x.circuit;
      if (!c) return BPGPU_E_ARG;
      if (x.nb && (!x.proofs || !x.init_states || !x.rho || (c->m && !x.commitments) || (screened && !x.ok))) return BPGPU_E_ARG;
      CK(gadget_label_rule(c, x.gadget_label, !(c->nchi > 1 || (c->nchi != 0) != (x.gadget_label != nullptr))));
      if (!wire_dims(x.proof_len, &dims[i].two_phase, &dims[i].k)) return BPGPU_E_LEN;
      CK(verify_shape(c, g, x.n1, dims[i].k));
      shape[i] = QueueShape{x.nb, verify_nvar(c, dims[i].k)};
    }
    return BPGPU_OK;
  }
  int prepare(bpgpu_ctx *ctx) {
    CK(sqrt_tab_locked(ctx));
    sqrt_tab = ctx->sqrt_tab;
    return wire_schedules_locked(ctx, G, dims, ngroups, sched);
  }
  // an undecodable proof or an identity at a validated point is malformed input: `bit`
  int front(bpgpu_ctx *ln, const MixSeg *segs, size_t nseg, int bit, MixSegIn *in) const {
    return wire_front_locked(ln, G, dims, sched, sqrt_tab, segs, nseg, bit, in);
  }
  // decodes the segment again, on its own (the lane's workspace has moved on since the check); it is the rare path and keeps the
  // one-circuit call's schedule cache
  int per_proof(bpgpu_ctx *ln, const MixSeg &sg) const {
    const Group &x = G[sg.gi];
    const size_t lo = sg.lo, m = x.circuit->m;
    return verify_wire_locked(ln, g, x.circuit, sg.cnt, x.n1, x.proof_len, (const uint8_t *)x.proofs + lo * x.proof_len,
                              m ? (const uint8_t *)x.commitments + lo * m * 32 : nullptr, (const uint8_t *)x.init_states + lo * 32,
                              (int32_t *)x.ok + lo, x.gadget_label, sqrt_tab);
  }
  static void fields(const Group &x, Group &d, StageField *f) {
    f[0] = StageField{x.proofs, &d.proofs, x.nb * x.proof_len};
    f[1] = StageField{x.commitments, &d.commitments, x.commitments ? x.nb * x.circuit->m * 32 : 0};
    f[2] = StageField{x.init_states, &d.init_states, x.nb * 32};
    f[3] = StageField{x.rho, &d.rho, x.nb * 32};
  }
};
}

/* ---- the drivers, the host staging and the entry helpers of both kinds ---- */
extern "C++" {   // (templates, in the middle of the C ABI)
// the sum of the checks' points; an empty queue gives the identity
template <class Kind> static int queue_combined_locked(bpgpu_ctx *ctx, Kind &q, void *partial_xy) {
  std::vector<MixSeg> segs;
  std::vector<MixCheck> checks;
  // (checks cut at the segment cap only; each picks its own MSM route)
  bpqueue::mixed_plan(q.shape, q.ngroups, (size_t)-1, (size_t)-1, BPGPU_MIXED_MAX_SEGMENTS, segs, checks);
  CK(flag_reset(ctx));
  if (checks.empty()) { HIPCK(ctx, hipMemsetAsync(partial_xy, 0, 64, ctx->st)); return BPGPU_OK; }
  CK(q.prepare(ctx));
  void *dpart = partial_xy;
  if (checks.size() > 1) CK(ws_get(ctx, WS_SCREEN_PART, checks.size() * 64, &dpart));
  for (size_t ci = 0; ci < checks.size(); ci++) {
    MixSegIn in[BPGPU_MIXED_MAX_SEGMENTS];
    CK(q.front(ctx, segs.data() + checks[ci].first, checks[ci].nseg, 1, in));      // bit 1, as verify_mixed's own malformed input
    CK(mixed_run_locked(ctx, q.g, in, checks[ci].nseg, (uint8_t *)dpart + 64 * ci, nullptr));
  }
  int *dbad2;
  if (checks.size() > 1) {       // the checks' partials are valid points: their sum cannot raise the flag (a separate one all the same)
    CK(ws_get(ctx, WS_SCREEN_FLAG, 256, (void **)&dbad2));
    points_sum(ctx->st, (const Words8 *)dpart, checks.size(), (Words8 *)partial_xy, dbad2);
  }
  mixed_poison(ctx->st, ctx->d_flag, (Words8 *)partial_xy);
  return launch_ok(ctx);
}
// the checks screened over the lanes (screen_locked); a failing check takes the per-proof path segment by segment
template <class Kind> static int queue_screened_locked(bpgpu_ctx *ctx, Kind &q, size_t *fallback_batches) {
  std::vector<MixSeg> segs;
  std::vector<MixCheck> checks;
  // proofs per check: BPGPU_OPT_SCREEN_BATCH, and at most 2^16 proof points (the one-instance bucket pipeline of k_pip2.hip)
  bpqueue::mixed_plan(q.shape, q.ngroups, (size_t)ctx->opt[BPGPU_OPT_SCREEN_BATCH], (size_t)1 << 16, BPGPU_MIXED_MAX_SEGMENTS, segs, checks);
  if (checks.empty()) return BPGPU_OK;
  CK(q.prepare(ctx));                         // on ctx->st, before screen_locked forks the lanes from it
  // a check's flag holds malformed input (bit 2 from the front) and zero weights
  auto check = [&](bpgpu_ctx *ln, size_t ci, void *partial) -> int {
    MixSegIn in[BPGPU_MIXED_MAX_SEGMENTS];
    CK(flag_reset(ln));
    CK(q.front(ln, segs.data() + checks[ci].first, checks[ci].nseg, 2, in));
    return mixed_run_locked(ln, q.g, in, checks[ci].nseg, partial, ln->d_flag);
  };
  auto accept = [&](size_t ci) -> int {
    const MixSeg *sg = segs.data() + checks[ci].first;
    for (size_t s = 0; s < checks[ci].nseg; s++)
      if (hipMemsetD32Async((hipDeviceptr_t)((int32_t *)q.G[sg[s].gi].ok + sg[s].lo), 1, sg[s].cnt, ctx->st) != hipSuccess) return BPGPU_E_DEVICE;
    return BPGPU_OK;
  };
  auto fallback = [&](bpgpu_ctx *ln, size_t ci) -> int {
    const MixSeg *sg = segs.data() + checks[ci].first;
    for (size_t s = 0; s < checks[ci].nseg; s++) CK(q.per_proof(ln, sg[s]));
    return BPGPU_OK;
  };
  return screen_locked(ctx, checks.size(), Kind::screened_name, fallback_batches, check, accept, fallback);
}
// host forms: every group's operands go up once (WS_MIXED_STAGE; one verdict region per group after its operands), and the queue
// moves on to the copies D that hold the device addresses
template <class Kind> static int queue_stage_locked(bpgpu_ctx *ctx, Kind &q, std::vector<typename Kind::Group> &D) {
  constexpr size_t NF = Kind::NFIELDS;
  StageField f[NF];
  size_t bytes[NF + 1], off[NF + 1], tot = 0;
  D.assign(q.G, q.G + q.ngroups);
  auto layout = [&](size_t i) {
    Kind::fields(q.G[i], D[i], f);
    for (size_t j = 0; j < NF; j++) bytes[j] = f[j].bytes;
    bytes[NF] = q.G[i].nb * 4;
    bpqueue::stage_layout(bytes, NF + 1, off, &tot);
  };
  for (size_t i = 0; i < q.ngroups; i++) layout(i);
  void *base;
  CK(ws_get(ctx, WS_MIXED_STAGE, tot, &base));
  tot = 0;
  for (size_t i = 0; i < q.ngroups; i++) {
    layout(i);
    for (size_t j = 0; j < NF; j++)
      if (f[j].src) { CK(h2d(ctx, (uint8_t *)base + off[j], f[j].src, f[j].bytes)); *f[j].dst = (uint8_t *)base + off[j]; }
    D[i].ok = (uint8_t *)base + off[NF];
  }
  q.G = D.data();
  return BPGPU_OK;
}
template <class Kind>
static int queue_combined_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, const typename Kind::Group *groups, size_t ngroups, void *partial_xy,
                                bool dev) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !partial_xy) return BPGPU_E_ARG;
    Kind q{g, groups, ngroups};
    CK(q.validate(false));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    if (dev) return queue_combined_locked(ctx, q, partial_xy);
    std::vector<typename Kind::Group> D;
    CK(queue_stage_locked(ctx, q, D));
    void *dout;
    CK(ws_get(ctx, WS_ARG4, 64, &dout));
    CK(queue_combined_locked(ctx, q, dout));
    CK(d2h(ctx, partial_xy, dout, 64));
    HIPCK(ctx, hipStreamSynchronize(ctx->st));
    return BPGPU_OK;
  });
}
template <class Kind>
static int queue_screened_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, const typename Kind::Group *groups, size_t ngroups,
                                size_t *fallback_batches, bool dev) {
  return noexcept_abi([&]() -> int {
    if (fallback_batches) *fallback_batches = 0;
    if (!ctx) return BPGPU_E_ARG;
    Kind q{g, groups, ngroups};
    CK(q.validate(true));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    if (dev) return queue_screened_locked(ctx, q, fallback_batches);
    std::vector<typename Kind::Group> D;
    CK(queue_stage_locked(ctx, q, D));
    CK(queue_screened_locked(ctx, q, fallback_batches));
    for (size_t i = 0; i < ngroups; i++) CK(d2h(ctx, groups[i].ok, D[i].ok, groups[i].nb * 4));
    HIPCK(ctx, hipStreamSynchronize(ctx->st));
    return BPGPU_OK;
  });
}
}  // extern "C++"
int bpgpu_r1cs_verify_mixed_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                         void *partial_xy_dev) {
  return queue_combined_entry<DecodedQueue>(ctx, g, groups, ngroups, partial_xy_dev, true);
}
int bpgpu_r1cs_verify_mixed_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                     uint8_t partial_xy[64]) {
  return queue_combined_entry<DecodedQueue>(ctx, g, groups, ngroups, partial_xy, false);
}
int bpgpu_r1cs_verify_mixed_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                         size_t *fallback_batches) {
  return queue_screened_entry<DecodedQueue>(ctx, g, groups, ngroups, fallback_batches, true);
}
int bpgpu_r1cs_verify_mixed_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                     size_t *fallback_batches) {
  return queue_screened_entry<DecodedQueue>(ctx, g, groups, ngroups, fallback_batches, false);
}
int bpgpu_r1cs_verify_mixed_wire_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                              void *partial_xy_dev) {
  return queue_combined_entry<WireQueue>(ctx, g, groups, ngroups, partial_xy_dev, true);
}
int bpgpu_r1cs_verify_mixed_wire_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                          uint8_t partial_xy[64]) {
  return queue_combined_entry<WireQueue>(ctx, g, groups, ngroups, partial_xy, false);
}
int bpgpu_r1cs_verify_mixed_wire_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                              size_t *fallback_batches) {
  return queue_screened_entry<WireQueue>(ctx, g, groups, ngroups, fallback_batches, true);
}
int bpgpu_r1cs_verify_mixed_wire_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                          size_t *fallback_batches) {
  return queue_screened_entry<WireQueue>(ctx, g, groups, ngroups, fallback_batches, false);
}

/* ---------------------------------------------------------------- IPP prover session */
// (ctx->mu held) the session's buffers go back to the context's pool
static void ipp_free_all(bpgpu_ctx *ctx, bpgpu_ipp *s) {
  void *all[] = {s->a[0], s->a[1], s->b[0], s->b[1], s->G[0], s->G[1], s->H[0], s->H[1], s->Q, s->Gf, s->Hf, s->t1, s->t2, s->t3, s->t4,
                 s->cLR, s->uu, s->res, s->sums, s->out_xy, s->mpts, s->msc, s->cG, s->cH, s->w, s->trip};
  for (void *p : all) pool_release(ctx, p);
  delete s;
}
// a session under construction: freed on the way out of its entry point (under the lock that entry point holds) unless it is
// released to the caller
namespace { struct IppFree { bpgpu_ctx *ctx; void operator()(bpgpu_ipp *s) const { ipp_free_all(ctx, s); } }; }
using IppOwner = std::unique_ptr<bpgpu_ipp, IppFree>;
// A resident-generator session of nb proofs of length n (planes 3: nb counts the virtual provers of an authenticated one): its fields,
// this rank's shard, its buffers.  `own` holds whatever was allocated, also on failure.
static int ipp_gens_session(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, int planes, IppOwner &own) {
  bpgpu_ipp *s = new (std::nothrow) bpgpu_ipp();
  if (!s) return BPGPU_E_OOM;
  own.reset(s);
  s->nb = nb; s->n0 = s->n = n; s->gens = g; s->planes = planes;
  if (ctx->shard_world > 1) { shard_bounds(n, ctx->shard_rank, ctx->shard_world, &s->slo, &s->shi); s->with_q = ctx->shard_rank == 0; }
  const size_t tot = nb * n, half = nb * (n > 1 ? n / 2 : 1);
  PoolTake M{ctx};
  M(&s->a[0], tot * 32); M(&s->b[0], tot * 32); M(&s->a[1], half * 32); M(&s->b[1], half * 32);
  M(&s->cG, tot * 32); M(&s->cH, tot * 32); M(&s->w, nb * 32);
  M(&s->cLR, nb * 2 * 32); M(&s->uu, nb * 2 * 32);
  M(&s->sums, nb * 2 * sizeof(JacRaw)); M(&s->out_xy, nb * 2 * 64);
  M(&s->msc, nb * 2 * (2 + 2 * n) * 32);
  if (planes != 1) M(&s->trip, (nb / 3) * 2 * 9 * (n / 2 ? n / 2 : 1) * 32);   // the first round's triples, the largest
  return M.ok ? BPGPU_OK : BPGPU_E_OOM;
}
int bpgpu_ipp_begin(bpgpu_ctx *ctx, size_t nb, size_t n, const uint8_t *Q, const uint8_t *G_factors,
                    const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int shared_gens, const uint8_t *a,
                    const uint8_t *b, bpgpu_ipp **out) {
  if (!ctx || !out || !nb || !Q || !G_factors || !H_factors || !G || !H || !a || !b) return BPGPU_E_ARG;
  if (!n || (n & (n - 1))) return BPGPU_E_LEN;   // assert!(n.is_power_of_two()), inner_product_proof.rs:70
  *out = nullptr;
  // ONE proof over arbitrary generators (the reference's `ipp-prover` criterion bench, benches/inner_product.rs:34-64; the tail of a
  // vector-sharded proof): the literal schedule folds G and H every round -- two dependent 252-doubling chains, ~2.8 ms per round
  // however small n is.  Instead build fixed-base tables for THESE generators once (B = B_blinding = Q, w = 1) and run the
  // resident-generator session: a round becomes table lookups.  Same group elements, same bytes.  BPGPU_OPT_IPP_LITERAL keeps the
  // literal schedule (nb > 1 with per-proof Q always takes it).  The tables are per session (256 KB per generator at c = 8 up to
  // n = 1024, 32 KB at c = 4 above: 2 GB at n = 2^15) and their build grows with n, so the route is bounded: n <=
  // BPGPU_OPT_IPP_TABLE_MAX_N (default 2^16), tables + staging within half of the free device memory, and a table build that
  // runs out of memory falls back to the literal schedule, whose footprint is O(n).
  if (nb == 1 && n >= 2) {
    const int c = n <= 1024 ? 8 : 4;
    const size_t per_gen = (252 / c + 1) * ((size_t)1 << (c - 1)), ng = 2 + 2 * n;
    size_t stage_gens = ((size_t)8 << 30) / ((per_gen + 252 / c + 1) * sizeof(JacRaw));
    if (stage_gens > ng) stage_gens = ng;
    const size_t need = ng * per_gen * sizeof(AffDev) + stage_gens * (per_gen + 252 / c + 1) * sizeof(JacRaw) + ng * 192;
    size_t free_b = 0, total_b = 0;
    bool fits = false;
    { std::lock_guard<std::mutex> lk(ctx->mu);
      fits = !ctx->opt[BPGPU_OPT_IPP_LITERAL] && n <= (size_t)ctx->opt[BPGPU_OPT_IPP_TABLE_MAX_N] &&
             hipSetDevice(ctx->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= free_b / 2; }
    if (fits) {
      bpgpu_gens *g = nullptr;
      int rc = bpgpu_gens_create(ctx, G, H, n, Q, Q, c, &g);
      if (rc == BPGPU_OK) {
        uint8_t one[32] = {1};
        rc = bpgpu_ipp_begin_gens(ctx, g, 1, n, one, G_factors, H_factors, a, b, out);
        if (rc == BPGPU_OK) { (*out)->own_gens = g; return BPGPU_OK; }
        bpgpu_gens_destroy(ctx, g);
      }
      if (rc != BPGPU_E_OOM) return rc;     // out of memory: the literal schedule below
    }
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  IppOwner own(new (std::nothrow) bpgpu_ipp(), IppFree{ctx});
  bpgpu_ipp *s = own.get();
  if (!s) return BPGPU_E_OOM;
  s->nb = nb; s->n0 = s->n = n; s->shared_gens = shared_gens != 0;
  size_t tot = nb * n, gtot = shared_gens ? n : tot, half = nb * (n > 1 ? n / 2 : 1);
  // the points' boundary form; the staging buffer goes back to the pool once its conversion launches have completed
  struct Stage {
    bpgpu_ctx *ctx;
    uint8_t *p;
    ~Stage() { (void)hipStreamSynchronize(ctx->st); pool_release(ctx, p); }
  } stage{ctx, nullptr};
  PoolTake M{ctx};
  M(&s->a[0], tot * 32); M(&s->b[0], tot * 32); M(&s->a[1], half * 32); M(&s->b[1], half * 32);
  M(&s->G[0], (gtot > half ? gtot : half) * sizeof(AffDev)); M(&s->H[0], (gtot > half ? gtot : half) * sizeof(AffDev));
  M(&s->G[1], half * sizeof(AffDev)); M(&s->H[1], half * sizeof(AffDev));
  M(&s->Q, nb * sizeof(AffDev)); M(&s->Gf, tot * 32); M(&s->Hf, tot * 32);
  M(&s->t1, half * 32); M(&s->t2, half * 32); M(&s->t3, half * 32); M(&s->t4, half * 32);
  M(&s->cLR, nb * 2 * 32); M(&s->uu, nb * 2 * 32);
  M(&s->res, nb * 2 * (n + 1) * sizeof(JacRaw)); M(&s->sums, nb * 2 * sizeof(JacRaw));
  M(&s->out_xy, nb * 2 * 64);
  M(&s->mpts, nb * 2 * (n + 1) * sizeof(AffDev)); M(&s->msc, nb * 2 * (n + 1) * 32);
  M(&stage.p, (2 * gtot + nb) * 64);
  if (!M.ok) return BPGPU_E_OOM;
  uint8_t *dG = stage.p, *dH = dG + gtot * 64, *dQ = dH + gtot * 64;
  CK(upload_inputs(ctx, {{s->a[0], a, tot * 32}, {s->b[0], b, tot * 32}, {s->Gf, G_factors, tot * 32}, {s->Hf, H_factors, tot * 32},
                         {dG, G, gtot * 64}, {dH, H, gtot * 64}, {dQ, Q, nb * 64}}));
  scalars_check(ctx->st, s->a[0], tot, ctx->d_flag);
  scalars_check(ctx->st, s->b[0], tot, ctx->d_flag);
  scalars_check(ctx->st, s->Gf, tot, ctx->d_flag);
  scalars_check(ctx->st, s->Hf, tot, ctx->d_flag);
  points_from_boundary(ctx->st, (Words8 *)dG, s->G[0], gtot, ctx->d_flag);
  points_from_boundary(ctx->st, (Words8 *)dH, s->H[0], gtot, ctx->d_flag);
  points_from_boundary(ctx->st, (Words8 *)dQ, s->Q, nb, ctx->d_flag);
  CK(checked_inputs(ctx));
  *out = own.release();
  return BPGPU_OK;
}
int bpgpu_ipp_begin_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *w,
                         const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *a, const uint8_t *b,
                         bpgpu_ipp **out) {
  if (!ctx || !g || !out || !nb || !w || !G_factors || !H_factors || !a || !b) return BPGPU_E_ARG;
  if (!n || (n & (n - 1))) return BPGPU_E_LEN;   // assert!(n.is_power_of_two()), inner_product_proof.rs:70
  if (n > g->cap) return BPGPU_E_GENS;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  IppOwner own(nullptr, IppFree{ctx});
  CK(ipp_gens_session(ctx, g, nb, n, 1, own));
  bpgpu_ipp *s = own.get();
  const size_t tot = nb * n;
  CK(upload_inputs(ctx, {{s->a[0], a, tot * 32}, {s->b[0], b, tot * 32}, {s->cG, G_factors, tot * 32}, {s->cH, H_factors, tot * 32},
                         {s->w, w, nb * 32}}));
  scalars_check(ctx->st, s->a[0], tot, ctx->d_flag);
  scalars_check(ctx->st, s->b[0], tot, ctx->d_flag);
  scalars_check(ctx->st, s->cG, tot, ctx->d_flag);
  scalars_check(ctx->st, s->cH, tot, ctx->d_flag);
  scalars_check(ctx->st, s->w, nb, ctx->d_flag);
  CK(checked_inputs(ctx));
  *out = own.release();
  return BPGPU_OK;
}
void bpgpu_ipp_destroy(bpgpu_ctx *ctx, bpgpu_ipp *s) {
  if (!s || !ctx) return;        // (a session belongs to the context it was opened on)
  bpgpu_gens *own = s->own_gens;
  { std::lock_guard<std::mutex> lk(ctx->mu); hipStreamSynchronize(ctx->st); hipStreamSynchronize(ctx->st2); ipp_free_all(ctx, s); }
  if (own) bpgpu_gens_destroy(ctx, own);
}
size_t bpgpu_ipp_len(const bpgpu_ipp *s) { return s ? s->n : 0; }

/* c_L, c_R and the two MSMs of one round -- inner_product_proof.rs:87-114 (first) / :156-172.
 * Device part: out_xy[2p], out_xy[2p + 1] = L_p, R_p in boundary form (2 Words8 per point). */
// beaver: cLR already holds c_L, c_R (an authenticated session's Beaver combine, bpgpu_mpc_ipp_round)
static int ipp_round_dev(bpgpu_ctx *ctx, bpgpu_ipp *s, Words8 *out_xy, bool beaver = false) {
  hipStream_t st = ctx->st;
  const size_t nb = s->nb, n = s->n, h = n / 2, seg = 2 * h + 1;
  Words8 *a = s->a[s->cur], *b = s->b[s->cur];
  if (s->gens) {   // resident generators: two table-lookup MSMs over the original generators per proof
    if (!beaver) {
      sc_dot_batched(st, nb, h, a, n, b + h, n, s->cLR, 2);        // c_L = <a_L, b_R>
      sc_dot_batched(st, nb, h, a + h, n, b, n, s->cLR + 1, 2);    // c_R = <a_R, b_L>
    }
    ipp_gens_scalars(st, nb, s->n0, n, a, b, s->cG, s->cH, s->cLR, s->w, s->msc, s->slo, s->shi, s->with_q);
    {
      size_t chunks = fixed_msm_ipp_chunks(s->gens->c, s->n0, nb * 2);
      void *dpart = nullptr;
      if (chunks > 1) CK(ws_get(ctx, WS_MSM, nb * 2 * chunks * sizeof(JacRaw), &dpart));
      ProfScope ps(ctx, 21, st);
      // (out_xy == nullptr: the caller's fused round tail sums the chunk partials and converts the points itself)
      const bool tail_sums = !out_xy && chunks > 1 && chunks <= 256;
      fixed_msm_ipp(st, s->gens->c, s->gens->table, s->n0, s->gens->cap, n, (const uint32_t *)s->msc, s->sums, nb * 2, (JacRaw *)dpart, !tail_sums);
      s->tail_partials = tail_sums ? (const JacRaw *)dpart : nullptr;
      s->tail_chunks = tail_sums ? chunks : 0;
    }
    if (out_xy) jac_to_boundary(st, s->sums, out_xy, nb * 2);
    return launch_ok(ctx);
  }
  const AffDev *G = s->G[s->cur], *H = s->H[s->cur];
  const bool shared = s->first && s->shared_gens;
  const size_t gouter = shared ? 0 : n;
  sc_dot_batched(st, nb, h, a, n, b + h, n, s->cLR, 2);        // c_L = <a_L, b_R>
  sc_dot_batched(st, nb, h, a + h, n, b, n, s->cLR + 1, 2);    // c_R = <a_R, b_L>
  const Words8 *sLa = a, *sLb = b + h, *sRa = a + h, *sRb = b;
  size_t so = n;   // outer stride (Words8) of the scalar sources
  if (s->first) {  // fold the factors into the scalars, :90-114
    sc_mul_strided(st, nb, h, a, n, 1, s->Gf + h, s->n0, 1, s->t1);       // a_L * G_factors[n..2n]
    sc_mul_strided(st, nb, h, b + h, n, 1, s->Hf, s->n0, 1, s->t2);       // b_R * H_factors[0..n]
    sc_mul_strided(st, nb, h, a + h, n, 1, s->Gf, s->n0, 1, s->t3);       // a_R * G_factors[0..n]
    sc_mul_strided(st, nb, h, b, n, 1, s->Hf + h, s->n0, 1, s->t4);       // b_L * H_factors[n..2n]
    sLa = s->t1; sLb = s->t2; sRa = s->t3; sRb = s->t4; so = h;
  }
  const size_t pip_min = (size_t)ctx->opt[BPGPU_OPT_IPP_PIPPENGER_MIN];
  {
    // make the 2 nb MSM instances contiguous: L = [a_L | b_R | c_L] x [G_R | H_L | Q], then R = [a_R | b_L | c_R] x [G_L | H_R | Q]
    const size_t io = 2 * seg;
    gather_points(st, G + h, gouter, h, nb, s->mpts, io);            gather_scalars(st, sLa, so, h, nb, s->msc, io);
    gather_points(st, H, gouter, h, nb, s->mpts + h, io);            gather_scalars(st, sLb, so, h, nb, s->msc + h, io);
    gather_points(st, s->Q, 1, 1, nb, s->mpts + 2 * h, io);          gather_scalars(st, s->cLR, 2, 1, nb, s->msc + 2 * h, io);
    gather_points(st, G, gouter, h, nb, s->mpts + seg, io);          gather_scalars(st, sRa, so, h, nb, s->msc + seg, io);
    gather_points(st, H + h, gouter, h, nb, s->mpts + seg + h, io);  gather_scalars(st, sRb, so, h, nb, s->msc + seg + h, io);
    gather_points(st, s->Q, 1, 1, nb, s->mpts + seg + 2 * h, io);    gather_scalars(st, s->cLR + 1, 2, 1, nb, s->msc + seg + 2 * h, io);
  }
  // long rounds: the bucket method, one batched launch chain for all instances; short ones: a Straus lane per term and a sum per instance
  const uint32_t *msc = (const uint32_t *)s->msc;
  CK(msm_tail(ctx, nb * 2, seg, pip_min, s->mpts, msc, straus_dense(s->mpts, msc), s->res, s->sums));
  jac_to_boundary(st, s->sums, out_xy, nb * 2);
  return launch_ok(ctx);
}
int bpgpu_ipp_round(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *L, uint8_t *R) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !L || !R || s->planes != 1) return BPGPU_E_ARG;   // (shares: c_L, c_R need Beaver triples, bpgpu_mpc_ipp_round)
    if (s->n < 2) return BPGPU_E_LEN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    CK(ipp_round_dev(ctx, s, s->out_xy));
    return download_pairs(ctx, s->out_xy, s->nb, 1, L, R);
  });
}
/* fold_witness with the round's challenges -- inner_product_proof.rs:125-146 (first) / :183-184 */
// device part of the fold: du / dui = the round's challenges and their inverses (nb each) already in HBM
static int ipp_fold_dev(bpgpu_ctx *ctx, bpgpu_ipp *s, Words8 *du, Words8 *dui) {
  hipStream_t st = ctx->st;
  const size_t nb = s->nb, n = s->n, h = n / 2;
  const int cur = s->cur, nxt = cur ^ 1;
  if (s->gens) {
    ipp_gens_fold(st, nb, s->n0, n, du, dui, s->cG, s->cH);
    fold_scalars_batched(st, nb, h, du, dui, s->a[cur], s->b[cur], s->a[nxt], s->b[nxt]);
    s->cur = nxt; s->n = h; s->first = false;
    return launch_ok(ctx);
  }
  const AffDev *G = s->G[cur], *H = s->H[cur];
  const bool shared = s->first && s->shared_gens;
  const size_t gouter = shared ? 0 : n;
  JacRaw *fres = s->res;   // reuse: nb x h (G) then nb x h (H)
  StrausArgs g{}, hh{};
  g.pts[0] = G; g.pts[1] = G + h; hh.pts[0] = H; hh.pts[1] = H + h;
  for (int j = 0; j < 2; j++) { g.pt_stride[j] = hh.pt_stride[j] = 1; g.pt_outer[j] = hh.pt_outer[j] = gouter; }
  g.inner = hh.inner = h;
  if (s->first) {   // G_i <- G_factors_i * G_i folded into the fold scalars, :125-134
    sc_mul_strided(st, nb, h, s->Gf, s->n0, 1, dui, 1, 0, s->t1);       // u^-1 * gf_i
    sc_mul_strided(st, nb, h, s->Gf + h, s->n0, 1, du, 1, 0, s->t2);    // u    * gf_{h+i}
    sc_mul_strided(st, nb, h, s->Hf, s->n0, 1, du, 1, 0, s->t3);        // u    * hf_i
    sc_mul_strided(st, nb, h, s->Hf + h, s->n0, 1, dui, 1, 0, s->t4);   // u^-1 * hf_{h+i}
    g.sc[0] = (uint32_t *)s->t1; g.sc[1] = (uint32_t *)s->t2; hh.sc[0] = (uint32_t *)s->t3; hh.sc[1] = (uint32_t *)s->t4;
    for (int j = 0; j < 2; j++) { g.sc_stride[j] = hh.sc_stride[j] = 8; g.sc_outer[j] = hh.sc_outer[j] = h * 8; }
  } else {
    g.sc[0] = (uint32_t *)dui; g.sc[1] = (uint32_t *)du; hh.sc[0] = (uint32_t *)du; hh.sc[1] = (uint32_t *)dui;
    for (int j = 0; j < 2; j++) { g.sc_stride[j] = hh.sc_stride[j] = 0; g.sc_outer[j] = hh.sc_outer[j] = 8; }
  }
  // the G and the H fold are independent 252-doubling chains: run them side by side on the context's two streams
  void *dstr, *dstr2;
  CK(straus_ws(ctx, 2, nb * h, &dstr));
  CK(ws_get(ctx, WS_MSM, straus_scratch_bytes(2, nb * h), &dstr2));
  hipStream_t st2 = ctx->st2;
  CK(side_fork(ctx));
  straus(st, 2, g, fres, nb * h, dstr);
  straus(st2, 2, hh, fres + nb * h, nb * h, dstr2);
  // when the input generators are shared the folded ones become per-proof: write them to buffer nxt
  batch_normalize(st, fres, s->G[nxt], nb * h, 8);
  batch_normalize(st2, fres + nb * h, s->H[nxt], nb * h, 8);
  CK(side_done(ctx));
  fold_scalars_batched(st, nb, h, du, dui, s->a[cur], s->b[cur], s->a[nxt], s->b[nxt]);
  CK(side_join(ctx));
  s->cur = nxt; s->n = h; s->first = false;
  return launch_ok(ctx);
}
// per-proof 32-byte values repeated for the three planes of each proof (authenticated sessions)
static std::vector<uint8_t> bcast3(const uint8_t *src, size_t nproofs) {
  std::vector<uint8_t> out(nproofs * 3 * 32);
  for (size_t v = 0; v < 3 * nproofs; v++) memcpy(&out[32 * v], src + 32 * (v / 3), 32);
  return out;
}
int bpgpu_ipp_fold(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *u, const uint8_t *u_inv) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !u || !u_inv) return BPGPU_E_ARG;
    if (s->n < 2) return BPGPU_E_LEN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nb = s->nb;
    Words8 *du = s->uu, *dui = s->uu + nb;
    CK(flag_reset(ctx));
    std::vector<uint8_t> b3;
    if (s->planes != 1) {   // authenticated session: one challenge per proof, broadcast to its three planes
      if (s->masked) return BPGPU_E_ARG;     // a masked round has not been completed by bpgpu_mpc_ipp_round
      b3 = bcast3(u, nb / 3);
      const std::vector<uint8_t> bi = bcast3(u_inv, nb / 3);
      b3.insert(b3.end(), bi.begin(), bi.end());
      CK(h2d(ctx, du, b3.data(), 2 * nb * 32));   // (du, dui adjacent; the flag's read below waits for the copy)
    } else {
      CK(h2d(ctx, du, u, nb * 32));
      CK(h2d(ctx, dui, u_inv, nb * 32));
    }
    scalars_check(ctx->st, s->uu, 2 * nb, ctx->d_flag);
    CK(checked_inputs(ctx));            // before the session state advances
    return ipp_fold_dev(ctx, s, du, dui);
  });
}
/* InnerProductProof::create's whole round loop on the device (SURVEY 8f N1 applied to the prover): per round the
 * L, R MSMs, transcript.append_point("L"), ("R"), challenge_scalar("u") (inner_product_proof.rs:119-123,177-181)
 * with the keccak hash chain in a kernel, u^-1 and the fold -- no host round trip between rounds. */
// the k rounds on states, L / R and (optional) per-round challenge arrays that are already in HBM (ctx->mu held; asynchronous):
// dlr: k x nb x (L, R) boundary points, round-major; uch: k arrays of nb, u_1..u_k (nullptr: not kept); dzero: a 4-byte scratch flag
static int ipp_rounds_fs_dev(bpgpu_ctx *ctx, bpgpu_ipp *s, size_t k, void *dstates, void *dlr, Words8 *uch, void *dzero) {
  const size_t nb = s->nb;
  Words8 *dui = s->uu + nb;
  ProfSpan span(ctx, 20, ctx->st);
  for (size_t r = 0; r < k; r++) {
    Words8 *lr = (Words8 *)dlr + r * nb * 4;             // 2 points x 2 Words8 per proof
    Words8 *du = uch ? uch + r * nb : s->uu;
    if (s->gens) {   // resident generators: point conversion, the three transcript steps and u^-1 in ONE launch (k_ipp_round_tail)
      CK(ipp_round_dev(ctx, s, nullptr));
      ipp_round_tail(ctx->st, nb, s->sums, (uint64_t *)dstates, lr, du, dui, s->tail_partials, s->tail_chunks);
    } else {
      CK(ipp_round_dev(ctx, s, lr));
      ipp_round_challenge(ctx->st, nb, (uint64_t *)dstates, lr, du);
      HIPCK(ctx, hipMemcpyAsync(dui, du, nb * 32, hipMemcpyDeviceToDevice, ctx->st));
      batch_inverse(ctx->st, dui, nb, (int *)dzero);       // challenges are non-zero up to 2^-252
    }
    CK(ipp_fold_dev(ctx, s, du, dui));
  }
  return BPGPU_OK;
}
int bpgpu_ipp_run_fs(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *states_in, uint8_t *L_out, uint8_t *R_out,
                     uint8_t *a_out, uint8_t *b_out, uint8_t *states_out) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !states_in || !a_out || !b_out || s->planes != 1) return BPGPU_E_ARG;
    if (s->shi != (size_t)-1) return BPGPU_E_ARG;    // a sharded session's L, R are partial sums: its rounds need the ranks' exchange
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nb = s->nb;
    size_t k = 0;
    for (size_t t = s->n; t > 1; t >>= 1) k++;
    if (k && (!L_out || !R_out)) return BPGPU_E_ARG;
    void *dstates, *dlr, *dzero;
    CK(ws_get(ctx, WS_FS_STAGE, nb * 32, &dstates));
    CK(ws_get(ctx, WS_FS_CH, (k ? k : 1) * nb * 128, &dlr));
    CK(ws_get(ctx, WS_PROOF_BAD, 4, &dzero));
    CK(h2d(ctx, dstates, states_in, nb * 32));
    CK(ipp_rounds_fs_dev(ctx, s, k, dstates, dlr, nullptr, dzero));
    // proof-major outputs: L_out[p][r], R_out[p][r]
    return download_pairs(ctx, dlr, nb, k, L_out, R_out,
                          {{a_out, s->a[s->cur], nb * 32}, {b_out, s->b[s->cur], nb * 32}, {states_out, dstates, states_out ? nb * 32 : 0}});
  });
}
/* final a, b -- inner_product_proof.rs:187-192 */
// The generators a resident-generator session has folded SO FAR, as points: G'_t = sum_{i = t mod n} cG[i] G_i (and H'), n = the
// session's current length.  For n == 1 this is the pair (G', H') the remaining state (a, b) refers to -- what a rank of a
// vector-sharded IPP (sharding.sharded_ipp_create: SURVEY 8e.2) hands to the final log2(ranks) rounds.  Only n == 1 is exposed.
int bpgpu_ipp_folded_gens(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *G_out, uint8_t *H_out) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !G_out || !H_out || !s->gens) return BPGPU_E_ARG;
    if (s->n != 1) return BPGPU_E_LEN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nb = s->nb, n0 = s->n0, per = 2 + 2 * n0;
    // MSM 2p over [B, Bb, G.., H..]: scalars cG[p] on the G block; MSM 2p + 1: cH[p] on the H block
    HIPCK(ctx, hipMemsetAsync(s->msc, 0, nb * 2 * per * 32, ctx->st));
    HIPCK(ctx, hipMemcpy2DAsync((uint8_t *)s->msc + 2 * 32, 2 * per * 32, s->cG, n0 * 32, n0 * 32, nb, hipMemcpyDeviceToDevice, ctx->st));
    HIPCK(ctx, hipMemcpy2DAsync((uint8_t *)s->msc + (per + 2 + n0) * 32, 2 * per * 32, s->cH, n0 * 32, n0 * 32, nb, hipMemcpyDeviceToDevice, ctx->st));
    CK(msm_gens_dev(ctx, s->gens, 2 * nb, n0, (const uint32_t *)s->msc, s->sums, ctx->st));
    jac_to_boundary(ctx->st, s->sums, s->out_xy, 2 * nb);
    CK(launch_ok(ctx));
    return download_pairs(ctx, s->out_xy, nb, 1, G_out, H_out);
  });
}
int bpgpu_ipp_finish(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *a_out, uint8_t *b_out) {
  if (!ctx || !s || !a_out || !b_out) return BPGPU_E_ARG;
  if (s->n != 1) return BPGPU_E_LEN;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (s->planes != 1) {   // authenticated planes leave in ark-ff Montgomery form, as every share of the two-party calls
    HIPCK(ctx, hipSetDevice(ctx->device));
    Words8 *t = s->out_xy;   // nb x 2 points = 4 nb words: room for a and b
    CK(flag_reset(ctx));
    scalars_to_ark(ctx->st, s->a[s->cur], t, s->nb, ctx->d_flag);
    scalars_to_ark(ctx->st, s->b[s->cur], t + s->nb, s->nb, ctx->d_flag);
    CK(launch_ok(ctx));
    CK(d2h(ctx, a_out, t, s->nb * 32));
    CK(d2h(ctx, b_out, t + s->nb, s->nb * 32));
    HIPCK(ctx, hipStreamSynchronize(ctx->st));
    return BPGPU_OK;
  }
  CK(d2h(ctx, a_out, s->a[s->cur], s->nb * 32));
  CK(d2h(ctx, b_out, s->b[s->cur], s->nb * 32));
  HIPCK(ctx, hipStreamSynchronize(ctx->st));
  return BPGPU_OK;
}

/* ---------------------------------------------------------------- R1CS prover polynomials */
/* One call = prover.rs:587-619: flattened_constraints(z), exp_y / exp_y_inv, the l/r coefficient
 * vectors and t_1..t_6 (util.rs:152-170) for nb provers of one circuit; then prover.rs:659-672
 * (l(x), r(x), padding) once the host transcript has produced x. */
struct bpgpu_prover {
  size_t nb = 0, n = 0, m = 0;
  int32_t *polys = nullptr;   // [6][nb][n][9]
  Words8 *y = nullptr;        // nb
  // resident-witness sessions (bpgpu_r1cs_prover_commit): the witness and blinding planes, nb x wn plain canonical words, stay in
  // HBM from the phase commitments to the polynomial build
  size_t wn = 0;
  Words8 *aL = nullptr, *aR = nullptr, *aO = nullptr, *sL = nullptr, *sR = nullptr;
  Words8 *yinv = nullptr;     // nb (set by bpgpu_r1cs_prover_session_polys)
  // authenticated sessions (bpgpu_mpc_prover_commit): nb above counts VIRTUAL provers, 3 per proof (share, MAC, modifier planes)
  int planes = 1;
  const bpgpu_gens *g = nullptr;        // the generators of the commitments (T points of bpgpu_mpc_prover_polys_finish)
  Words8 *trip = nullptr, *wv = nullptr; // the polynomial build's Beaver triples (plain) and wV (proofs x m), mask -> finish
  bool finished = false;
  // a session of bpgpu_r1cs_prove_fs2_begin, until _finish consumes it: four arrays over the nb provers -- the chain states after the
  // gadget challenge (32 B each), the gadget challenges, the phase-1 blinding factors (3 each, plain), A_I1 A_O1 S1 (3 x 64 B each)
  Words8 *fs2 = nullptr;
  const bpgpu_circuit *fs2_c = nullptr;   // the circuit _begin was given
};
static void prover_free_all(bpgpu_ctx *ctx, bpgpu_prover *s) {   // ctx->mu held
  void *all[] = {s->polys, s->y, s->aL, s->aR, s->aO, s->sL, s->sR, s->yinv, s->trip, s->wv, s->fs2};
  for (void *p : all) pool_release(ctx, p);
  delete s;
}
namespace { struct ProverFree { bpgpu_ctx *ctx; void operator()(bpgpu_prover *s) const { prover_free_all(ctx, s); } }; }
using ProverOwner = std::unique_ptr<bpgpu_prover, ProverFree>;   // a session under construction (as IppOwner)

/* ---- what the three polynomial builds share (prover_polys_impl: staged witness; prover_session_polys_locked and
 * bpgpu_mpc_prover_polys_mask: resident witness) --------------------------------------------------------------------------- */
// polys and y of the session's s->nb (virtual) provers, from the pool
static int polys_alloc(bpgpu_ctx *ctx, bpgpu_prover *s, size_t n) {
  PoolTake M{ctx};
  M(&s->polys, (6 * s->nb * (n ? n : 1) * 9) * 4); M(&s->y, s->nb * 32);
  return M.ok ? BPGPU_OK : BPGPU_E_OOM;
}
// the z-power table of nb proofs into WS_ZPOW (a parametric circuit's carries one block per gadget challenge); dz, dchi: validated
static int zpow_build(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const Words8 *dz, const Words8 *dchi, const int32_t **dzp) {
  const size_t qz = (1 + c->nchi) * (c->q ? c->q : 1);
  void *p;
  CK(ws_get(ctx, WS_ZPOW, nb * qz * 9 * 4, &p));
  zpow_table(ctx->st, nb, c->q, dz, 8, (int32_t *)p, c->nchi, dchi);
  *dzp = (const int32_t *)p;
  return BPGPU_OK;
}
// A build on a resident-witness session (ctx->mu held): until it is kept, what it allocated goes back to the pool on the way out and
// the session stays where it was -- the call may be repeated.
namespace {
struct PolysBuild {
  bpgpu_ctx *ctx;
  bpgpu_prover *s;
  bool kept = false;
  ~PolysBuild() {
    if (kept) return;
    for (void **p : {(void **)&s->polys, (void **)&s->y, (void **)&s->yinv, (void **)&s->trip, (void **)&s->wv}) { pool_release(ctx, *p); *p = nullptr; }
  }
};
}  // namespace
// Its head: polys, y, y^-1 from the pool; y (one per virtual prover) into the session, z and the gadget challenges (one set per proof)
// into WS_ARG0 / WS_CHI; all of them validated.
struct PolyChallenges { const Words8 *z, *chi; };
static int session_polys_begin(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z, const uint8_t *chi,
                               PolyChallenges *ch, OperandSrc from = {}) {
  const size_t nv = s->nb, nb = nv / (size_t)s->planes;
  CK(polys_alloc(ctx, s, c->n));
  if (!pool_alloc(ctx, (void **)&s->yinv, nv * 32)) return BPGPU_E_OOM;
  void *dz, *dchi = nullptr;
  CK(ws_get(ctx, WS_ARG0, nb * 32, &dz));
  if (c->nchi) CK(ws_get(ctx, WS_CHI, nb * c->nchi * 32, &dchi));
  CK(upload_inputs(ctx, {{s->y, y, nv * 32}, {dz, z, nb * 32}, {dchi, chi, nb * c->nchi * 32}}, from));
  scalars_check(ctx->st, s->y, nv, ctx->d_flag);
  scalars_check(ctx->st, (const Words8 *)dz, nb, ctx->d_flag);
  if (c->nchi) scalars_check(ctx->st, (const Words8 *)dchi, nb * c->nchi, ctx->d_flag);
  ch->z = (const Words8 *)dz; ch->chi = (const Words8 *)dchi;
  return BPGPU_OK;
}
// ... and what its polynomial kernel reads besides the witness: y^-1 (prover.rs:593; a zero challenge raises the flag: E_ARG), z powers
static int session_polys_powers(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const PolyChallenges &ch, const int32_t **dzp) {
  HIPCK(ctx, hipMemcpyAsync(s->yinv, s->y, s->nb * 32, hipMemcpyDeviceToDevice, ctx->st));
  batch_inverse(ctx->st, s->yinv, s->nb, ctx->d_flag);
  return zpow_build(ctx, c, s->nb / (size_t)s->planes, ch.z, ch.chi, dzp);
}
static int prover_polys_impl(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *y, const uint8_t *y_inv,
                             const uint8_t *z, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                             const uint8_t *s_L, const uint8_t *s_R, uint8_t *t_coeffs, uint8_t *wV,
                             bpgpu_prover **out, bool ark) {
  if (!ctx || !c || !out || !nb || !y || !y_inv || !z || !t_coeffs || (c->m && !wV)) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;      // the prover knows its gadget challenges when it builds the rows: numeric circuits only
  size_t n = c->n, m = c->m;
  if (n && (!a_L || !a_R || !a_O || !s_L || !s_R)) return BPGPU_E_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  ProverOwner own(new (std::nothrow) bpgpu_prover(), ProverFree{ctx});
  bpgpu_prover *s = own.get();
  if (!s) return BPGPU_E_OOM;
  s->nb = nb; s->n = n; s->m = m;
  CK(polys_alloc(ctx, s, n));
  // y, y^-1 and z arrive with the witness, in the witness's form: one staging block, one validation (or conversion) launch
  void *din, *dout;
  size_t tot = nb * n;
  CK(ws_get(ctx, WS_ARG0, (3 * nb + 5 * tot) * 32, &din));
  CK(ws_get(ctx, WS_ARG1, (nb * 6 + nb * m) * 32, &dout));
  Words8 *w = (Words8 *)din;
  Words8 *dy = w, *dyi = w + nb, *dz = w + 2 * nb, *dL = w + 3 * nb, *dR = dL + tot, *dO = dR + tot, *dsL = dO + tot, *dsR = dsL + tot;
  Words8 *dt = (Words8 *)dout, *dwV = dt + nb * 6;
  CK(upload_inputs(ctx, {{dy, y, nb * 32}, {dyi, y_inv, nb * 32}, {dz, z, nb * 32}, {dL, a_L, tot * 32}, {dR, a_R, tot * 32},
                         {dO, a_O, tot * 32}, {dsL, s_L, tot * 32}, {dsR, s_R, tot * 32}}));
  if (ark) scalars_from_ark(ctx->st, w, w, 3 * nb + 5 * tot, ctx->d_flag);
  else scalars_check(ctx->st, w, 3 * nb + 5 * tot, ctx->d_flag);
  HIPCK(ctx, hipMemcpyAsync(s->y, dy, nb * 32, hipMemcpyDeviceToDevice, ctx->st));
  const int32_t *dzp;
  CK(zpow_build(ctx, c, nb, dz, nullptr, &dzp));   // (parametric circuits are rejected above: the prover builds numeric rows)
  prover_polys(ctx->st, circuit_dev(c), nb, dy, dyi, dL, dR, dO, dsL, dsR, dzp, s->polys, dwV);
  prover_tcoeffs(ctx->st, nb, n, s->polys, dt);
  CK(checked_download(ctx, {{t_coeffs, dt, nb * 6 * 32}, {wV, dwV, nb * m * 32}}));
  *out = own.release();
  return BPGPU_OK;
}
int bpgpu_r1cs_prover_polys(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *y, const uint8_t *y_inv,
                            const uint8_t *z, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                            const uint8_t *s_L, const uint8_t *s_R, uint8_t *t_coeffs, uint8_t *wV,
                            bpgpu_prover **out) {
  return prover_polys_impl(ctx, c, nb, y, y_inv, z, a_L, a_R, a_O, s_L, s_R, t_coeffs, wV, out, false);
}
int bpgpu_r1cs_prover_polys_ark(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *y, const uint8_t *y_inv,
                                const uint8_t *z, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                                const uint8_t *s_L, const uint8_t *s_R, uint8_t *t_coeffs, uint8_t *wV,
                                bpgpu_prover **out) {
  return prover_polys_impl(ctx, c, nb, y, y_inv, z, a_L, a_R, a_O, s_L, s_R, t_coeffs, wV, out, true);
}
int bpgpu_r1cs_prover_eval(bpgpu_ctx *ctx, bpgpu_prover *s, size_t padded_n, const uint8_t *x, uint8_t *l_vec,
                           uint8_t *r_vec) {
  if (!ctx || !s || !x || !l_vec || !r_vec || s->planes != 1 || s->fs2) return BPGPU_E_ARG;   // (fs2: _finish owns such a session's rest)
  if (padded_n < s->n || (padded_n & (padded_n - 1))) return BPGPU_E_LEN;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *dx, *dout;
  size_t nb = s->nb;
  CK(ws_get(ctx, WS_ARG0, nb * 32, &dx));
  CK(ws_get(ctx, WS_ARG1, 2 * nb * padded_n * 32, &dout));
  Words8 *dl = (Words8 *)dout, *dr = dl + nb * padded_n;
  CK(flag_reset(ctx));
  CK(h2d(ctx, dx, x, nb * 32));
  scalars_check(ctx->st, (Words8 *)dx, nb, ctx->d_flag);
  prover_eval(ctx->st, nb, s->n, padded_n, (Words8 *)dx, s->y, s->polys, dl, dr);
  return checked_download(ctx, {{l_vec, dl, nb * padded_n * 32}, {r_vec, dr, nb * padded_n * 32}});
}
/* prover.rs:659-708 without leaving the device: l(x), r(x) with their padding, the G/H factors and the
 * resident-generator IPP session that consumes them */
// (x, u, w: one per virtual prover; an authenticated session (planes 3) evaluates with k_mpc_eval and takes its own y^-1)
// the session and its launches (ctx->mu held; no host-side wait): `own` holds the session, also on failure
static int prover_ipp_begin_core(bpgpu_ctx *ctx, bpgpu_prover *ps, const bpgpu_gens *g, size_t padded_n, size_t n1, const uint8_t *x,
                                 const uint8_t *u, const uint8_t *y_inv, const uint8_t *w, OperandSrc from, IppOwner &own) {
  const size_t nb = ps->nb, n = padded_n;
  CK(ipp_gens_session(ctx, g, nb, n, ps->planes, own));
  bpgpu_ipp *s = own.get();
  void *din;
  CK(ws_get(ctx, WS_ARG0, 3 * nb * 32, &din));
  Words8 *dx = (Words8 *)din, *du = dx + nb, *dyi = du + nb;
  CK(upload_inputs(ctx, {{dx, x, nb * 32}, {du, u, nb * 32}, {s->w, w, nb * 32}}, from));
  if (y_inv) CK(copy_in(ctx, dyi, y_inv, nb * 32, from.src_dev));
  else HIPCK(ctx, hipMemcpyAsync(dyi, ps->yinv, nb * 32, hipMemcpyDeviceToDevice, ctx->st));
  ProfSpan span(ctx, 19, ctx->st);
  scalars_check(ctx->st, dx, 3 * nb, ctx->d_flag);
  scalars_check(ctx->st, s->w, nb, ctx->d_flag);
  if (ps->planes != 1) mpc_eval(ctx->st, nb / 3, ps->n, n, dx, ps->y, ps->polys, s->a[0], s->b[0]);
  else prover_eval(ctx->st, nb, ps->n, n, dx, ps->y, ps->polys, s->a[0], s->b[0]);
  ipp_r1cs_factors(ctx->st, nb, n, n1, du, dyi, s->cG, s->cH);
  return BPGPU_OK;
}
static int prover_ipp_begin_impl(bpgpu_ctx *ctx, bpgpu_prover *ps, const bpgpu_gens *g, size_t padded_n, size_t n1,
                                 const uint8_t *x, const uint8_t *u, const uint8_t *y_inv, const uint8_t *w,
                                 bpgpu_ipp **out) {
  if (!padded_n || padded_n < ps->n || (padded_n & (padded_n - 1)) || n1 > ps->n) return BPGPU_E_LEN;
  if (padded_n > g->cap) return BPGPU_E_GENS;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  IppOwner own(nullptr, IppFree{ctx});
  CK(prover_ipp_begin_core(ctx, ps, g, padded_n, n1, x, u, y_inv, w, {}, own));
  CK(checked_inputs(ctx));
  *out = own.release();
  return BPGPU_OK;
}
int bpgpu_r1cs_prover_ipp_begin(bpgpu_ctx *ctx, bpgpu_prover *ps, const bpgpu_gens *g, size_t padded_n, size_t n1,
                                const uint8_t *x, const uint8_t *u, const uint8_t *y_inv, const uint8_t *w,
                                bpgpu_ipp **out) {
  if (!ctx || !ps || !g || !x || !u || (!y_inv && !ps->yinv) || !w || !out || !ps->polys || ps->planes != 1 || ps->fs2) return BPGPU_E_ARG;
  return prover_ipp_begin_impl(ctx, ps, g, padded_n, n1, x, u, y_inv, w, out);
}
void bpgpu_prover_destroy(bpgpu_ctx *ctx, bpgpu_prover *s) {
  if (!s || !ctx) return;        // (a session belongs to the context it was opened on)
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipStreamSynchronize(ctx->st);
  prover_free_all(ctx, s);
}

/* ---- resident-witness prover sessions: prover.rs:457-494 / :519-565 (phase commitments) and :587-619 (polynomials) with the
 * witness uploaded ONCE and the blinding vectors optionally drawn on the device ------------------------------------------ */
// planes = 3: an authenticated session (bpgpu_mpc_prover_commit), nb = 3 x proofs virtual provers
// the launches of one commitment phase on a session whose fields are set (ctx->mu held; no host-side wait): the operands from host
// memory or HBM (`from`), the blindings bl_pitch bytes apart (3 x 32: the staged calls' packed triples), *dcommit = nb x 3 boundary points
static int prover_commit_core(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover *s, size_t nb, size_t n_new, const uint8_t *a_L,
                              const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys,
                              const uint8_t *blindings, size_t bl_pitch, OperandSrc from, Words8 **dcommit) {
  const bool explicit_vec = s_L && s_R;
  const size_t wn0 = s->wn, wn = wn0 + n_new;
  // new planes of nb x wn; the multipliers of the earlier phase are carried over
  Words8 *pl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  Words8 **old[5] = {&s->aL, &s->aR, &s->aO, &s->sL, &s->sR};
  const size_t tot_new = nb * n_new;
  void *din = nullptr, *drows = nullptr, *dres = nullptr, *dout = nullptr;
  CK(ws_get(ctx, WS_ARG0, (5 * tot_new + 4 * nb) * 32, &din));
  CK(ws_get(ctx, WS_ARG1, nb * 3 * (2 + 2 * wn) * 32, &drows));
  CK(ws_get(ctx, WS_ARG4, nb * 3 * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG5, nb * 3 * 64, &dout));
  if (n_new) {
    auto drop = [&](int rc) { for (auto p : pl) pool_release(ctx, p); return rc; };   // (until the session takes the new planes)
    PoolTake M{ctx};
    for (int i = 0; i < 5; i++) M(&pl[i], nb * wn * 32);
    if (!M.ok) return drop(BPGPU_E_OOM);
    if (wn0) for (int i = 0; i < 5; i++)
      if (hipMemcpy2DAsync(pl[i], wn * 32, *old[i], wn0 * 32, wn0 * 32, nb, hipMemcpyDeviceToDevice, ctx->st) != hipSuccess) return drop(BPGPU_E_DEVICE);
    for (int i = 0; i < 5; i++) { pool_release(ctx, *old[i]); *old[i] = pl[i]; }   // (stream-ordered: any reuse runs after the copies)
    s->wn = wn;
  }
  // staging: [a_L | a_R | a_O | (s_L | s_R)] nb x n_new each, then blindings nb x 3 (all ark), then the keys nb x 32 bytes (raw)
  Words8 *w = (Words8 *)din;
  const size_t nvec = explicit_vec ? 5 : 3;
  Words8 *dbl = w + nvec * tot_new, *dkeys = dbl + 3 * nb;
  const uint8_t *src[5] = {a_L, a_R, a_O, s_L, s_R};
  if (from.reset) CK(flag_reset(ctx));
  for (size_t i = 0; i < nvec && n_new; i++) CK(copy_in(ctx, w + i * tot_new, src[i], tot_new * 32, from.src_dev));
  if (bl_pitch == 3 * 32) CK(copy_in(ctx, dbl, blindings, nb * 3 * 32, from.src_dev));
  else HIPCK(ctx, hipMemcpy2DAsync(dbl, 3 * 32, blindings, bl_pitch, 3 * 32, nb, from.src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->st));
  if (n_new && !explicit_vec) CK(copy_in(ctx, dkeys, vector_keys, nb * 32, from.src_dev));
  ProfSpan span(ctx, 16, ctx->st);
  if (n_new) {
    if (wn0 == 0) {          // contiguous planes: convert straight into them
      for (size_t i = 0; i < nvec; i++) scalars_from_ark(ctx->st, w + i * tot_new, *old[i], tot_new, ctx->d_flag);
    } else {
      scalars_from_ark(ctx->st, w, w, nvec * tot_new, ctx->d_flag);
      for (size_t i = 0; i < nvec; i++)
        HIPCK(ctx, hipMemcpy2DAsync(*old[i] + wn0, wn * 32, w + i * tot_new, n_new * 32, n_new * 32, nb, hipMemcpyDeviceToDevice, ctx->st));
    }
    if (!explicit_vec) blind_vectors(ctx->st, dkeys, nb, n_new, s->sL, s->sR, wn, wn0);
  }
  scalars_from_ark(ctx->st, dbl, dbl, 3 * nb, ctx->d_flag);
  size_t slo = 0, shi = wn;
  if (ctx->shard_world > 1) shard_bounds(wn, ctx->shard_rank, ctx->shard_world, &slo, &shi);   // this rank's generators: partial commitments
  commit_rows(ctx->st, nb, wn, wn0, wn, s->aL, s->aR, s->aO, s->sL, s->sR, dbl, (Words8 *)drows, slo, shi, ctx->shard_rank == 0);
  // (three classes of rows per prover -- A_I, A_O: bit vectors; S: dense -- so that a wave of the MSM-per-lane walk holds one class)
  CK(msm_gens_dev(ctx, g, nb * 3, wn, (const uint32_t *)drows, (JacRaw *)dres, ctx->st, WS_MSM, 0, 3));
  jac_to_boundary(ctx->st, (JacRaw *)dres, (Words8 *)dout, nb * 3);
  *dcommit = (Words8 *)dout;
  return BPGPU_OK;
}
static int prover_commit_impl(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover **session, size_t nb, size_t n_new,
                              const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                              const uint8_t *vector_keys, const uint8_t *blindings, uint8_t *commitments, int planes) {
  if (!ctx || !g || !session || !nb || !blindings || !commitments) return BPGPU_E_ARG;
  if (*session && (*session)->planes != planes) return BPGPU_E_ARG;   // no mixing of single-party and authenticated calls
  if (*session && (*session)->fs2) return BPGPU_E_ARG;                // opened by bpgpu_r1cs_prove_fs2_begin: _finish commits its phase 2
  if (n_new && (!a_L || !a_R || !a_O)) return BPGPU_E_ARG;
  const bool explicit_vec = s_L && s_R;
  if (n_new && (explicit_vec == (vector_keys != nullptr) || (!s_L) != (!s_R))) return BPGPU_E_ARG;   // exactly one source of s_L, s_R
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  bpgpu_prover *s = *session;
  const bool fresh = s == nullptr;
  if (!fresh && s->nb != nb) return BPGPU_E_LEN;
  const size_t wn0 = fresh ? 0 : s->wn, wn = wn0 + n_new;
  if (wn > g->cap) return BPGPU_E_GENS;
  if (fresh) {
    s = new (std::nothrow) bpgpu_prover();
    if (!s) return BPGPU_E_OOM;
    s->nb = nb; s->planes = planes; s->g = g;
  }
  ProverOwner own(fresh ? s : nullptr, ProverFree{ctx});   // only a fresh session is freed on failure
  Words8 *dout = nullptr;
  CK(prover_commit_core(ctx, g, s, nb, n_new, a_L, a_R, a_O, s_L, s_R, vector_keys, blindings, 3 * 32, {}, &dout));
  CK(checked_download(ctx, {{commitments, dout, nb * 3 * 64}}));
  (void)own.release();
  *session = s;
  return BPGPU_OK;
}
int bpgpu_r1cs_prover_commit(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover **session, size_t nb, size_t n_new,
                             const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                             const uint8_t *vector_keys, const uint8_t *blindings, uint8_t *commitments) {
  return prover_commit_impl(ctx, g, session, nb, n_new, a_L, a_R, a_O, s_L, s_R, vector_keys, blindings, commitments, 1);
}
static int prover_session_polys_locked(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                       const uint8_t *chi, uint8_t *t_coeffs, uint8_t *wV);
int bpgpu_r1cs_prover_session_polys(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                    uint8_t *t_coeffs, uint8_t *wV) {
  if (!ctx || !s || !c || !y || !z || !t_coeffs || (c->m && !wV) || s->planes != 1 || s->fs2) return BPGPU_E_ARG;
  if (c->nchi) return BPGPU_E_ARG;
  return prover_session_polys_locked(ctx, s, c, y, z, nullptr, t_coeffs, wV);
}
int bpgpu_r1cs_prover_session_polys_param(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                          const uint8_t *gadget_challenges, uint8_t *t_coeffs, uint8_t *wV) {
  if (!ctx || !s || !c || !y || !z || !t_coeffs || (c->m && !wV) || s->planes != 1 || s->fs2) return BPGPU_E_ARG;
  if (!c->nchi || !gadget_challenges) return BPGPU_E_ARG;
  return prover_session_polys_locked(ctx, s, c, y, z, gadget_challenges, t_coeffs, wV);
}
// the launches of the polynomial build (ctx->mu held; no host-side wait): *dt = nb x 6 t coefficients, *dwV = nb x m, in WS_ARG1
static int session_polys_core(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z, const uint8_t *chi,
                              OperandSrc from, Words8 **dt_out, Words8 **dwV_out) {
  const size_t nb = s->nb, n = c->n, m = c->m;
  void *dout;
  CK(ws_get(ctx, WS_ARG1, (nb * 6 + nb * m) * 32, &dout));
  Words8 *dt = (Words8 *)dout, *dwV = dt + nb * 6;
  PolyChallenges ch;
  CK(session_polys_begin(ctx, s, c, y, z, chi, &ch, from));
  ProfSpan span(ctx, 17, ctx->st);
  const int32_t *dzp;
  CK(session_polys_powers(ctx, s, c, ch, &dzp));
  prover_polys(ctx->st, circuit_dev(c), nb, s->y, s->yinv, s->aL, s->aR, s->aO, s->sL, s->sR, dzp, s->polys, dwV);
  prover_tcoeffs(ctx->st, nb, n, s->polys, dt);
  *dt_out = dt; *dwV_out = dwV;
  return BPGPU_OK;
}
static int prover_session_polys_locked(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                       const uint8_t *chi, uint8_t *t_coeffs, uint8_t *wV) {
  if (c->n != s->wn || s->polys) return BPGPU_E_LEN;     // the circuit's multipliers are the session's; one polynomial build per session
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t nb = s->nb, n = c->n, m = c->m;
  PolysBuild build{ctx, s};
  Words8 *dt, *dwV;
  CK(session_polys_core(ctx, s, c, y, z, chi, {}, &dt, &dwV));
  CK(checked_download(ctx, {{t_coeffs, dt, nb * 6 * 32}, {wV, dwV, nb * m * 32}}));
  build.kept = true;
  s->n = n; s->m = m;
  return BPGPU_OK;
}
/* ---- Prover::prove (r1cs/prover.rs:412-727) for nb provers with the Fiat-Shamir transcript on the device: in ONE call for a circuit
 * without randomized constraints (bpgpu_r1cs_prove_fs), in TWO around the host's gadget for a two-phase circuit with one gadget
 * challenge, or with the nchi <= 8 of a circuit that carries its labels (bpgpu_circuit_set_gadget_labels) -- bpgpu_r1cs_prove_fs2_begin =
 * :420-501, the phase-1 commitments and the chain up to the last gadget challenge; _finish = :515-727.
 * From a proof's last commitment phase on both are ONE chain, prove_fs_chain_locked: the commitments, the polynomial build, the T
 * commitments, t(x) and the blindings, the IPP session and its rounds on the context's stream, with the transcript on the device
 * between them (k_prover_transcript, a slice of the schedule each time) -- the host neither hashes nor waits until the proofs are
 * complete.  The stages are the cores of the staged entry points above, fed from HBM; what is new are the transcript slices and the
 * links of k_prove_fs.hip.  A two-phase session carries the chain state, the challenge, the phase-1 blinding factors and commitments
 * from _begin to _finish in HBM: _finish_dev may follow _begin_dev on the stream without a wait. ----------------------------------- */
namespace {
// The operands and results of an entry point as it was given them -- in host memory, or in HBM (the *_dev forms) -- and, for the
// _locked functions, always in HBM.  states_in: the one-phase call's and _begin's (the session carries the chain to _finish)
struct ProveFsIo {
  const void *states_in, *a_L, *a_R, *a_O, *s_L, *s_R, *vector_keys, *v_blinding, *blindings;
  void *proof_points, *proof_scalars, *wire, *challenges_out, *states_out;
};
struct ProveFs2BeginIo {
  const void *states_in;
  const uint8_t *gadget_label;   // host memory in every form
  const void *a_L, *a_R, *a_O, *s_L, *s_R, *vector_keys, *blindings;
  void *commitments, *chi_out, *states_out;
};
struct ProveFsDims { size_t n, m, padded_n, k; };
struct Fs2Arrays { uint64_t *states; Words8 *chi, *bl1, *A1; };   // per prover: 1 state, nchi challenges, 3 blinding factors, 3 points
// resident step list; slice j = steps [cut[j], cut[j + 1]); labels: the circuit's label table behind the steps, or null
struct ProverSched { const TrStep *steps; const int *cut; const uint8_t *labels; };
// what the one-phase call | a two-phase _finish hand the chain
struct ProveFsPhase {
  uint64_t *states;               // the chain states: the workspace's | the session's
  ProverSched sched;              // the one-phase | the two-phase schedule ...
  int slice;                      // ... and its slice that absorbs this phase's commitments and draws y, z: 0 | 1
  const Words8 *chi, *bl1, *A1;   // nullptr | the session's gadget challenges (nb x nchi), phase-1 blinding factors and phase-1 commitments
  size_t n_commit, n1;            // multipliers to commit: n | n - n1;  the IPP's G_factors = [1; n1] ++ [u; ..]: n | n1
};
struct ProveFsWs {   // the chain's workspace
  uint64_t *states;                     // WS_PFS_CH: nb chain states (the one-phase call's), ...
  Words8 *ch, *uch;                     // ... y z u x w: nb each; then u_1..u_k
  Words8 *bl, *vb, *rows, *tb2, *sc3;   // WS_PFS_SC: nb x 8 blindings, nb x m v_blinding, nb x 10 T rows, nb tb2, nb x 3 t_x t_x_blinding e_blinding
  Words8 *T;                            // WS_PFS_PTS: nb x 5 T points, ...
  JacRaw *Tres;                         // ... and their Jacobian sums
  void *lr, *zero;                      // WS_FS_CH: the rounds' L, R;  WS_PROOF_BAD
};
}  // namespace
static const uint8_t *u8(const void *p) { return (const uint8_t *)p; }
static ProveFsDims prove_fs_dims(const bpgpu_circuit *c) {
  ProveFsDims d{c->n, c->m, 1, 0};
  while (d.padded_n < d.n) { d.padded_n <<= 1; d.k++; }
  return d;
}
static size_t fs2_words(size_t nb, size_t nchi) { return nb * (1 + nchi + 3 + 6); }
static Fs2Arrays fs2_arrays(const bpgpu_prover *s) {
  const size_t nb = s->nb, nchi = s->fs2_c->nchi;
  return {(uint64_t *)s->fs2, s->fs2 + nb, s->fs2 + (1 + nchi) * nb, s->fs2 + (4 + nchi) * nb};
}
static int prove_fs_workspace(bpgpu_ctx *ctx, size_t nb, const ProveFsDims &d, ProveFsWs *w) {
  void *dchs, *dscs, *dpts;
  CK(ws_get(ctx, WS_PFS_CH, nb * (1 + 5 + d.k) * 32, &dchs));
  CK(ws_get(ctx, WS_PFS_SC, nb * (8 + d.m + 10 + 1 + 3) * 32, &dscs));
  CK(ws_get(ctx, WS_PFS_PTS, nb * 5 * (64 + sizeof(JacRaw)), &dpts));
  CK(ws_get(ctx, WS_FS_CH, (d.k ? d.k : 1) * nb * 128, &w->lr));
  CK(ws_get(ctx, WS_PROOF_BAD, 4, &w->zero));
  w->states = (uint64_t *)dchs;
  w->ch = (Words8 *)dchs + nb; w->uch = w->ch + 5 * nb;
  w->bl = (Words8 *)dscs; w->vb = w->bl + 8 * nb; w->rows = w->vb + nb * d.m; w->tb2 = w->rows + 10 * nb; w->sc3 = w->tb2 + nb;
  w->T = (Words8 *)dpts; w->Tres = (JacRaw *)(w->T + nb * 5 * 2);
  return BPGPU_OK;
}
// the prover's transcript schedule of (two_phase, m, padded_n) in HBM (ctx->mu held) -- c: the two-phase circuit (its nchi gadget
// steps, and its label table behind the steps if it has one), null for one phase.  Each kind keeps its own resident copy and key:
// a context that alternates between the two uploads, and waits, only when a kind's shape (or the circuit's labels) changes
static int prover_schedule(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t m, size_t padded_n, ProverSched *out) {
  constexpr size_t ROOM = PROVER_SCHEDULE_MAX + gadget_label_slots(8);
  const bool two_phase = c != nullptr;
  const size_t nchi = c ? c->nchi : 0;
  const uint8_t *labels = c ? circuit_labels(c) : nullptr;
  const size_t label_id = labels ? c->labels_id : 0;
  void *dsteps;
  CK(ws_get(ctx, two_phase ? WS_PFS_SCHED2 : WS_PFS_SCHED, ROOM * sizeof(TrStep), &dsteps));
  auto &e = ctx->psched[two_phase];
  if (e.key[0] != m || e.key[1] != padded_n || e.key[2] != nchi || e.key[3] != label_id) {
    TrStep steps[ROOM];
    memset(steps, 0, sizeof steps);
    const int len = prover_transcript_schedule(steps, nchi, m, padded_n, e.cut);
    static_assert(PROVER_SCHEDULE_MAX >= 23 + 8, "the two-phase schedule has 23 steps and one per gadget challenge");
    if (labels) memcpy(steps + PROVER_SCHEDULE_MAX, labels, nchi * GADGET_LABEL_BYTES);
    e.key[0] = (size_t)-1;                       // (nothing resident if the upload fails)
    HIPCK(ctx, hipMemcpyAsync(dsteps, steps, (labels ? ROOM : (size_t)len) * sizeof(TrStep), hipMemcpyHostToDevice, ctx->st));
    HIPCK(ctx, hipStreamSynchronize(ctx->st));   // `steps` is a local
    e.key[0] = m; e.key[1] = padded_n; e.key[2] = nchi; e.key[3] = label_id;
  }
  *out = {(const TrStep *)dsteps, e.cut, labels ? (const uint8_t *)((const TrStep *)dsteps + PROVER_SCHEDULE_MAX) : nullptr};
  return BPGPU_OK;
}
// The chain from a proof's last commitment phase to its assembly (ctx->mu held, shapes checked; asynchronous).  `s` holds whatever was
// committed before (`ph`); the IPP session's buffers go back to the context's pool on the way out (stream-ordered reuse), as do `s`'s
// with its owner, whatever the outcome.
static int prove_fs_chain_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover *s, const ProveFsWs &w,
                                 const ProveFsIo &io, const ProveFsPhase &ph) {
  const ProveFsDims d = prove_fs_dims(c);
  const size_t nb = s->nb, m = d.m, k = d.k;
  hipStream_t st = ctx->st;
  const OperandSrc dev{true, false};                 // operands in HBM; ONE input flag for the whole chain
  const uint8_t *cy = (const uint8_t *)w.ch, *cz = (const uint8_t *)(w.ch + nb), *cu = (const uint8_t *)(w.ch + 2 * nb),
                *cx = (const uint8_t *)(w.ch + 3 * nb), *cw = (const uint8_t *)(w.ch + 4 * nb);
  auto transcript = [&](int slice, const Words8 *points, size_t npoints, const Words8 *scalars, size_t nscalars) {
    const int *cut = ph.sched.cut + ph.slice + slice;
    prover_transcript(st, nb, ph.sched.steps + cut[0], cut[1] - cut[0], ph.states, points, npoints, scalars, nscalars, w.ch);
  };
  IppOwner iown(nullptr, IppFree{ctx});
  {
    ProfScope link(ctx, 22, st);
    scalars_from_ark(st, (const Words8 *)io.blindings, w.bl, 8 * nb, ctx->d_flag);
    scalars_from_ark(st, (const Words8 *)io.v_blinding, w.vb, nb * m, ctx->d_flag);
  }
  // prover.rs:457-494 | :515-565: this phase's commitments A_I A_O S over G, H [n - n_commit, n).  Into the transcript: after
  // append_u64("m") (:420), as A_I1 A_O1 S1 before the 1-phase separator and the identity phase-2 points | as A_I2 A_O2 S2; y, z (:584-585)
  Words8 *dA;
  CK(prover_commit_core(ctx, g, s, nb, ph.n_commit, u8(io.a_L), u8(io.a_R), u8(io.a_O), u8(io.s_L), u8(io.s_R), u8(io.vector_keys), u8(io.blindings),
                        8 * 32, dev, &dA));
  {
    ProfScope link(ctx, 22, st);
    transcript(0, dA, 3, nullptr, 0);
  }
  // :587-640: y^-1, the flattened constraints (on the gadget challenge, if any), l / r coefficients, t_1..t_6;
  // T_i = t_i B + tb_i B_blinding; u, x
  Words8 *dt, *dwV;
  CK(session_polys_core(ctx, s, c, cy, cz, (const uint8_t *)ph.chi, dev, &dt, &dwV));
  s->n = d.n; s->m = m;
  {
    ProfScope link(ctx, 22, st);
    prove_fs_t_rows(st, nb, dt, w.bl, w.rows);
  }
  {
    ProfScope tmsm(ctx, 18, st);
    CK(msm_gens_dev(ctx, g, nb * 5, 0, (const uint32_t *)w.rows, w.Tres, st));
    jac_to_boundary(st, w.Tres, w.T, nb * 5);
  }
  {
    // :644-686: tb2 = <wV, v_blinding>, t_x, t_x_blinding, e_blinding (over both phases' blinding factors, if there are two); w; then
    // innerproduct_domain_sep (inner_product_proof.rs:72)
    ProfScope link(ctx, 22, st);
    transcript(1, w.T, 5, nullptr, 0);
    const bool coop = m > PROVE_FS_DOT_LANE_MAX;
    if (coop) sc_dot_batched(st, nb, m, dwV, m, w.vb, m, w.tb2, 1);
    prove_fs_glue(st, nb, m, (const Words8 *)cx, dt, w.bl, dwV, w.vb, coop ? w.tb2 : nullptr, w.sc3, ph.bl1 ? (const Words8 *)cu : nullptr, ph.bl1);
    transcript(2, nullptr, 0, w.sc3, 3);
  }
  // :687-708: l(x), r(x), the G / H factors, Q = w B; the k rounds (u_j kept for challenges_out)
  CK(prover_ipp_begin_core(ctx, s, g, d.padded_n, ph.n1, cx, cu, nullptr, cw, dev, iown));
  bpgpu_ipp *ipp = iown.get();
  CK(ipp_rounds_fs_dev(ctx, ipp, k, ph.states, w.lr, w.uch, w.zero));
  {
    ProfScope link(ctx, 22, st);
    ProveFsAssemble a{nb, k, ph.A1 ? ph.A1 : dA, w.T, (const Words8 *)w.lr, w.sc3, ipp->a[ipp->cur], ipp->b[ipp->cur], w.ch, w.uch, ph.states,
                      (Words8 *)io.proof_points, (Words8 *)io.proof_scalars, (Words8 *)io.challenges_out, (Words8 *)io.states_out, (uint8_t *)io.wire,
                      ph.A1 ? dA : nullptr};
    prove_fs_assemble(st, a);
  }
  return launch_ok(ctx);
}
/* ---- the host forms' staging (WS_PFS_STAGE) ---- */
// The operands, back to back in the order given (an absent one, of zero bytes, gets a null device pointer), then the results.  `placed`
// runs once the staging exists and before anything is enqueued; then the flag is reset and the operands are uploaded.
static int prove_fs_stage(bpgpu_ctx *ctx, size_t n_in, const void *const *in_host, const size_t *in_bytes, uint8_t **in_dev, size_t n_out,
                          const size_t *out_bytes, uint8_t **out_dev, const std::function<void()> &placed = nullptr) {
  size_t total = 0;
  for (size_t i = 0; i < n_in; i++) total += in_bytes[i];
  for (size_t i = 0; i < n_out; i++) total += out_bytes[i];
  void *dstage;
  CK(ws_get(ctx, WS_PFS_STAGE, total, &dstage));
  if (placed) placed();
  uint8_t *at = (uint8_t *)dstage;
  for (size_t i = 0; i < n_in; i++) { in_dev[i] = in_bytes[i] ? at : nullptr; at += in_bytes[i]; }
  for (size_t i = 0; i < n_out; i++) { out_dev[i] = at; at += out_bytes[i]; }
  CK(flag_reset(ctx));
  for (size_t i = 0; i < n_in; i++) CK(h2d(ctx, in_dev[i], in_host[i], in_bytes[i]));
  return BPGPU_OK;
}
// A proof call (the one-phase one, or _finish) from host memory: `a`'s nine operands of in_bytes each (states_in: none for _finish) and
// the five results -- proof_points, proof_scalars, challenges_out, states_out, then the wire form of wire_len bytes per proof, of
// odd length and therefore last; the optional ones are downloaded only when asked for -- around `run` on the staged Io
static int prove_fs_staged(bpgpu_ctx *ctx, size_t nb, size_t k, size_t wire_len, const ProveFsIo &a, const size_t (&in_bytes)[9],
                           const std::function<int(const ProveFsIo &)> &run, const std::function<void()> &placed = nullptr) {
  const void *in_host[9] = {a.states_in, a.a_L, a.a_R, a.a_O, a.s_L, a.s_R, a.vector_keys, a.v_blinding, a.blindings};
  const size_t out_bytes[5] = {nb * (11 + 2 * k) * 64, nb * 5 * 32, nb * (5 + k) * 32, nb * 32, a.wire ? nb * wire_len : 0};
  uint8_t *in[9], *out[5];
  CK(prove_fs_stage(ctx, 9, in_host, in_bytes, in, 5, out_bytes, out, placed));
  CK(run(ProveFsIo{in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], out[0], out[1], a.wire ? out[4] : nullptr, out[2], out[3]}));
  return checked_download(ctx, {{a.proof_points, out[0], out_bytes[0]}, {a.proof_scalars, out[1], out_bytes[1]},
                                {a.challenges_out, out[2], a.challenges_out ? out_bytes[2] : 0},
                                {a.states_out, out[3], a.states_out ? out_bytes[3] : 0}, {a.wire, out[4], out_bytes[4]}});
}
/* ---- one phase: bpgpu_r1cs_prove_fs ---- */
// the refusals that depend on shapes alone, before anything is launched (BPGPU_OK with nb == 0: nothing to do)
static int prove_fs_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const ProveFsIo &a) {
  if (!ctx || !g || !c) return BPGPU_E_ARG;
  CK(bpgpu_internal_prove_fs_shape(g, c, nb));
  if (!nb) return BPGPU_OK;
  if (!a.states_in || !a.a_L || !a.a_R || !a.a_O || !a.blindings || !a.proof_points || !a.proof_scalars || (c->m && !a.v_blinding)) return BPGPU_E_ARG;
  if ((!a.s_L) != (!a.s_R) || (a.s_L != nullptr) == (a.vector_keys != nullptr)) return BPGPU_E_ARG;   // exactly one source of s_L, s_R
  return BPGPU_OK;
}
// ctx->mu held, shapes checked, nb > 0; asynchronous.  The session lives until the last launch is enqueued: its buffers go back to
// the context's pool on the way out (stream-ordered reuse), whatever the outcome.
static int prove_fs_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const ProveFsIo &io) {
  if (ctx->shard_world > 1) return BPGPU_E_ARG;      // partial sums cannot be hashed: a sharded proof needs the ranks' exchange
  const ProveFsDims d = prove_fs_dims(c);
  ProveFsWs w;
  ProverSched sched;
  CK(prove_fs_workspace(ctx, nb, d, &w));
  CK(prover_schedule(ctx, nullptr, d.m, d.padded_n, &sched));
  bpgpu_prover *s = new (std::nothrow) bpgpu_prover();
  if (!s) return BPGPU_E_OOM;
  ProverOwner pown(s, ProverFree{ctx});
  s->nb = nb; s->planes = 1; s->g = g;
  CK(copy_in(ctx, w.states, io.states_in, nb * 32, true));
  return prove_fs_chain_locked(ctx, g, c, s, w, io, {w.states, sched, 0, nullptr, nullptr, nullptr, d.n, d.n});
}
static int prove_fs_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const ProveFsIo &a, bool dev) {
  return noexcept_abi([&]() -> int {
    CK(prove_fs_check(ctx, g, c, nb, a));
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->shard_world > 1) return BPGPU_E_ARG;
    if (!nb) return BPGPU_OK;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if (dev) {
      CK(flag_reset(ctx));   // the flag reports on the most recent *_dev call
      return prove_fs_locked(ctx, g, c, nb, a);
    }
    const ProveFsDims d = prove_fs_dims(c);
    const size_t tot = nb * d.n * 32;
    return prove_fs_staged(ctx, nb, d.k, 1 + 11 * 32 + (2 * d.k + 2) * 32, a,
                           {nb * 32, tot, tot, tot, a.s_L ? tot : 0, a.s_R ? tot : 0, a.vector_keys ? nb * 32 : 0, nb * d.m * 32, nb * 8 * 32},
                           [&](const ProveFsIo &io) { return prove_fs_locked(ctx, g, c, nb, io); });
  });
}
int bpgpu_r1cs_prove_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const void *states_in, const void *a_L,
                            const void *a_R, const void *a_O, const void *s_L, const void *s_R, const void *vector_keys,
                            const void *v_blinding, const void *blindings, void *proof_points, void *proof_scalars, void *wire,
                            void *challenges_out, void *states_out) {
  return prove_fs_entry(ctx, g, c, nb, {states_in, a_L, a_R, a_O, s_L, s_R, vector_keys, v_blinding, blindings, proof_points, proof_scalars, wire,
                                        challenges_out, states_out}, true);
}
int bpgpu_r1cs_prove_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const uint8_t *states_in, const uint8_t *a_L,
                        const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys,
                        const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire,
                        uint8_t *challenges_out, uint8_t *states_out) {
  return prove_fs_entry(ctx, g, c, nb, {states_in, a_L, a_R, a_O, s_L, s_R, vector_keys, v_blinding, blindings, proof_points, proof_scalars, wire,
                                        challenges_out, states_out}, false);
}
/* ---- two phases: bpgpu_r1cs_prove_fs2_begin, then _finish on its session ---- */
// the refusals that depend on shapes and arguments alone (BPGPU_OK with nb == 0: nothing to do)
static int prove_fs2_begin_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const ProveFs2BeginIo &a,
                                 bpgpu_prover **session) {
  if (!ctx || !g || !c || !session || *session) return BPGPU_E_ARG;
  CK(bpgpu_internal_prove_fs2_labels(c, a.gadget_label, false));
  if (!nb) return BPGPU_OK;
  if (n1 >= c->n) return BPGPU_E_LEN;        // (no second-phase commitments: the staged calls serve such provers)
  if (prove_fs_dims(c).padded_n > g->cap) return BPGPU_E_GENS;
  if (!a.states_in || (!a.gadget_label && !circuit_labels(c)) || !a.blindings) return BPGPU_E_ARG;
  if (n1 && (!a.a_L || !a.a_R || !a.a_O || (!a.s_L) != (!a.s_R) || (a.s_L != nullptr) == (a.vector_keys != nullptr))) return BPGPU_E_ARG;
  return BPGPU_OK;
}
// ctx->mu held, shapes checked, nb > 0; asynchronous.  `own` holds the session, also on failure.
static int prove_fs2_begin_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const ProveFs2BeginIo &io,
                                  ProverOwner &own) {
  const ProveFsDims d = prove_fs_dims(c);
  hipStream_t st = ctx->st;
  const OperandSrc dev{true, false};                 // operands in HBM; the caller has reset the input flag
  ProverSched sched;
  CK(prover_schedule(ctx, c, d.m, d.padded_n, &sched));
  bpgpu_prover *s = new (std::nothrow) bpgpu_prover();
  if (!s) return BPGPU_E_OOM;
  own.reset(s);
  s->nb = nb; s->planes = 1; s->g = g; s->fs2_c = c;
  if (!pool_alloc(ctx, (void **)&s->fs2, fs2_words(nb, c->nchi) * 32)) return BPGPU_E_OOM;
  const Fs2Arrays f = fs2_arrays(s);
  CK(copy_in(ctx, f.states, io.states_in, nb * 32, true));
  {
    ProfScope link(ctx, 22, st);
    scalars_from_ark(st, (const Words8 *)io.blindings, f.bl1, 3 * nb, ctx->d_flag);
  }
  // prover.rs:420-501: append_u64("m"), the phase-1 commitments, the 2-phase separator, the gadget's challenge
  const bool keys = n1 && !io.s_L;
  Words8 *dA;
  CK(prover_commit_core(ctx, g, s, nb, n1, u8(io.a_L), u8(io.a_R), u8(io.a_O), n1 ? u8(io.s_L) : nullptr, n1 ? u8(io.s_R) : nullptr,
                        keys ? u8(io.vector_keys) : nullptr, u8(io.blindings), 3 * 32, dev, &dA));
  {
    ProfScope link(ctx, 22, st);
    prover_transcript(st, nb, sched.steps + sched.cut[0], sched.cut[1] - sched.cut[0], f.states, dA, 3, nullptr, 0, nullptr, io.gadget_label,
                      f.chi, c->nchi, sched.labels);
  }
  HIPCK(ctx, hipMemcpyAsync(f.A1, dA, nb * 3 * 64, hipMemcpyDeviceToDevice, st));
  if (io.commitments) HIPCK(ctx, hipMemcpyAsync(io.commitments, dA, nb * 3 * 64, hipMemcpyDeviceToDevice, st));
  if (io.chi_out) HIPCK(ctx, hipMemcpyAsync(io.chi_out, f.chi, nb * c->nchi * 32, hipMemcpyDeviceToDevice, st));
  if (io.states_out) HIPCK(ctx, hipMemcpyAsync(io.states_out, f.states, nb * 32, hipMemcpyDeviceToDevice, st));   // (little-endian words)
  return launch_ok(ctx);
}
static int prove_fs2_begin_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const ProveFs2BeginIo &a,
                                 bpgpu_prover **session, bool dev) {
  return noexcept_abi([&]() -> int {
    CK(prove_fs2_begin_check(ctx, g, c, nb, n1, a, session));
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->shard_world > 1) return BPGPU_E_ARG;    // partial sums cannot be hashed
    if (!nb) return BPGPU_OK;
    HIPCK(ctx, hipSetDevice(ctx->device));
    ProverOwner own(nullptr, ProverFree{ctx});
    if (dev) {
      CK(flag_reset(ctx));   // the flag reports on the most recent *_dev call; _finish_dev adds to it: one flag for the pair
      CK(prove_fs2_begin_locked(ctx, g, c, nb, n1, a, own));
    } else {
      const size_t tot = nb * n1 * 32;
      const void *in_host[8] = {a.states_in, a.a_L, a.a_R, a.a_O, a.s_L, a.s_R, a.vector_keys, a.blindings};
      const size_t in_bytes[8] = {nb * 32, tot, tot, tot, n1 && a.s_L ? tot : 0, n1 && a.s_R ? tot : 0, n1 && a.vector_keys ? nb * 32 : 0,
                                  nb * 3 * 32};
      const size_t out_bytes[3] = {nb * 3 * 64, nb * c->nchi * 32, nb * 32};
      uint8_t *in[8], *out[3];
      CK(prove_fs_stage(ctx, 8, in_host, in_bytes, in, 3, out_bytes, out));
      CK(prove_fs2_begin_locked(ctx, g, c, nb, n1, {in[0], a.gadget_label, in[1], in[2], in[3], in[4], in[5], in[6], in[7], out[0], out[1], out[2]},
                                own));
      CK(checked_download(ctx, {{a.commitments, out[0], a.commitments ? out_bytes[0] : 0}, {a.chi_out, out[1], a.chi_out ? out_bytes[1] : 0},
                                {a.states_out, out[2], a.states_out ? out_bytes[2] : 0}}));
    }
    *session = own.release();
    return BPGPU_OK;
  });
}
int bpgpu_r1cs_prove_fs2_begin_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const void *states_in,
                                   const uint8_t gadget_label[32], const void *a_L, const void *a_R, const void *a_O, const void *s_L,
                                   const void *s_R, const void *vector_keys, const void *blindings, bpgpu_prover **session,
                                   void *commitments, void *gadget_challenges_out, void *states_out) {
  return prove_fs2_begin_entry(ctx, g, c, nb, n1, {states_in, gadget_label, a_L, a_R, a_O, s_L, s_R, vector_keys, blindings, commitments,
                                                   gadget_challenges_out, states_out}, session, true);
}
int bpgpu_r1cs_prove_fs2_begin(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const uint8_t *states_in,
                               const uint8_t gadget_label[32], const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                               const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *blindings,
                               bpgpu_prover **session, uint8_t *commitments, uint8_t *gadget_challenges_out, uint8_t *states_out) {
  return prove_fs2_begin_entry(ctx, g, c, nb, n1, {states_in, gadget_label, a_L, a_R, a_O, s_L, s_R, vector_keys, blindings, commitments,
                                                   gadget_challenges_out, states_out}, session, false);
}
// _finish's refusals: they leave the session open
static int prove_fs2_finish_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const ProveFsIo &a) {
  if (!ctx || !g || !c || !session || !*session) return BPGPU_E_ARG;
  const bpgpu_prover *s = *session;
  if (!s->fs2 || s->fs2_c != c || s->g != g) return BPGPU_E_ARG;   // opened by _begin, on this circuit and these generators
  if (!a.a_L || !a.a_R || !a.a_O || !a.blindings || !a.proof_points || !a.proof_scalars || (c->m && !a.v_blinding)) return BPGPU_E_ARG;
  if ((!a.s_L) != (!a.s_R) || (a.s_L != nullptr) == (a.vector_keys != nullptr)) return BPGPU_E_ARG;   // exactly one source of s_L, s_R
  return BPGPU_OK;
}
// ctx->mu held, arguments checked; asynchronous.  The session is `pown`'s: its buffers go back to the context's pool on the way out
// (stream-ordered reuse), whatever the outcome.
static int prove_fs2_finish_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, ProverOwner &pown, const ProveFsIo &io) {
  bpgpu_prover *s = pown.get();
  const ProveFsDims d = prove_fs_dims(c);
  const Fs2Arrays f = fs2_arrays(s);
  ProveFsWs w;
  ProverSched sched;
  CK(prover_schedule(ctx, c, d.m, d.padded_n, &sched));
  CK(prove_fs_workspace(ctx, s->nb, d, &w));
  return prove_fs_chain_locked(ctx, g, c, s, w, io, {f.states, sched, 1, f.chi, f.bl1, f.A1, d.n - s->wn, s->wn});
}
static int prove_fs2_finish_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const ProveFsIo &a,
                                  bool dev) {
  return noexcept_abi([&]() -> int {
    CK(prove_fs2_finish_check(ctx, g, c, session, a));
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->shard_world > 1) return BPGPU_E_ARG;
    HIPCK(ctx, hipSetDevice(ctx->device));
    ProverOwner pown(nullptr, ProverFree{ctx});
    auto take = [&] { pown.reset(*session); *session = nullptr; };   // from there on the session is consumed
    if (dev) {
      take();   // (no flag reset: what _begin_dev's operands raised stays raised -- the flag reports on the pair)
      return prove_fs2_finish_locked(ctx, g, c, pown, a);
    }
    const ProveFsDims d = prove_fs_dims(c);
    const size_t nb = (*session)->nb, tot = nb * (d.n - (*session)->wn) * 32;
    return prove_fs_staged(ctx, nb, d.k, 1 + 14 * 32 + (2 * d.k + 2) * 32, a,
                           {0, tot, tot, tot, a.s_L ? tot : 0, a.s_R ? tot : 0, a.vector_keys ? nb * 32 : 0, nb * d.m * 32, nb * 8 * 32},
                           [&](const ProveFsIo &io) { return prove_fs2_finish_locked(ctx, g, c, pown, io); }, take);
  });
}
int bpgpu_r1cs_prove_fs2_finish_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const void *a_L,
                                    const void *a_R, const void *a_O, const void *s_L, const void *s_R, const void *vector_keys,
                                    const void *v_blinding, const void *blindings, void *proof_points, void *proof_scalars, void *wire,
                                    void *challenges_out, void *states_out) {
  return prove_fs2_finish_entry(ctx, g, c, session, {nullptr, a_L, a_R, a_O, s_L, s_R, vector_keys, v_blinding, blindings, proof_points,
                                                     proof_scalars, wire, challenges_out, states_out}, true);
}
int bpgpu_r1cs_prove_fs2_finish(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const uint8_t *a_L,
                                const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys,
                                const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points, uint8_t *proof_scalars,
                                uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out) {
  return prove_fs2_finish_entry(ctx, g, c, session, {nullptr, a_L, a_R, a_O, s_L, s_R, vector_keys, v_blinding, blindings, proof_points,
                                                     proof_scalars, wire, challenges_out, states_out}, false);
}
/* ---- the step before Prover::prove: Prover::commit for every committed value (prover.rs:319-329) -- V = v B + v_blinding B_blinding
 * over the resident Pedersen pair and, optionally, the chain from Prover::new up to the last append_point("V") -- and one party's
 * local half of MpcProver::batch_commit_preshared (mpc_prover.rs:402-456), the same sums over the three planes. ------------------- */
namespace {
struct CommitIo { const void *v, *v_blinding, *states_in; void *V, *V_compressed, *states_out; };   // host memory, or HBM (the _dev form, the _locked function)
constexpr size_t COMMIT_VALUES_MAX = (size_t)1 << 30;   // commitments of one call (include/bpgpu.h)
}  // namespace
// the refusals that depend on the pointers alone
static int commit_values_check(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nv, size_t m, const CommitIo &a) {
  if (!ctx || !g) return BPGPU_E_ARG;
  if (nv && m && (!a.v || !a.v_blinding)) return BPGPU_E_ARG;
  if ((a.states_in != nullptr) != (a.states_out != nullptr)) return BPGPU_E_ARG;   // the chain's two ends go together
  if (!a.V && !a.V_compressed && !a.states_out) return BPGPU_E_ARG;
  return BPGPU_OK;
}
// ctx->mu held, arguments checked, nv > 0, every pointer in HBM; asynchronous.  nv virtual provers of m commitments each (nv = 3 nb
// for a party's planes), the chain -- if asked for -- over nchain = nv provers.  The points are the fixed-base launch with zero
// vector generators over rows of two scalars; the workspace goes back to the pool on the way out (stream-ordered reuse).
static int commit_values_locked(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nv, size_t m, const CommitIo &io) {
  const size_t tot = nv * m;
  hipStream_t st = ctx->st;
  PoolBlock ws(ctx);
  Words8 *dV = (Words8 *)io.V;
  if (tot) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // (rows of two scalars are at most 128 window pairs: fixed_msm_chunks gives 1 at every table width today, so `part` stays null
    // and the launch sums inside a block or a wave; the scratch follows the function in case its tuning changes)
    const size_t chunks = fixed_msm_chunks(g->c, 0, tot);
    const size_t b_rows = tot * 2 * sizeof(Words8), b_res = up(tot * sizeof(JacRaw)), b_part = chunks > 1 ? up(tot * chunks * sizeof(JacRaw)) : 0;
    if (!pool_alloc(ctx, &ws.p, b_rows + b_res + b_part + (dV ? 0 : tot * 64))) return BPGPU_E_OOM;
    uint8_t *at = (uint8_t *)ws.p;
    Words8 *rows = (Words8 *)at; at += b_rows;
    JacRaw *res = (JacRaw *)at; at += b_res;
    JacRaw *part = b_part ? (JacRaw *)at : nullptr; at += b_part;
    if (!dV) dV = (Words8 *)at;
    ProfScope points(ctx, 16, st);
    commit_value_rows(st, (const Words8 *)io.v, (const Words8 *)io.v_blinding, rows, tot, ctx->d_flag);
    fixed_msm(st, g->c, g->table, 0, g->cap, (const uint32_t *)rows, 2 * 8, res, tot, part);
    jac_to_boundary(st, res, dV, tot);
    if (io.V_compressed) points_compress(st, dV, (Words8 *)io.V_compressed, tot);
  }
  if (io.states_out) {
    ProfScope chain(ctx, 22, st);
    commit_transcript(st, nv, m, (const Words8 *)io.states_in, dV, (Words8 *)io.states_out);
  }
  return launch_ok(ctx);
}
static int commit_values_entry(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, int planes, size_t m, const CommitIo &a, bool dev) {
  return noexcept_abi([&]() -> int {
    CK(commit_values_check(ctx, g, nb, m, a));
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->shard_world > 1) return BPGPU_E_ARG;      // a commitment is one rank's: nothing of it is sharded
    if (nb > COMMIT_VALUES_MAX / planes || (m && nb * planes > COMMIT_VALUES_MAX / m)) return BPGPU_E_LEN;
    if (!nb) return BPGPU_OK;
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nv = nb * planes, tot = nv * m;
    CK(flag_reset(ctx));   // (the _dev form: the flag reports on the most recent *_dev call)
    if (dev) return commit_values_locked(ctx, g, nv, m, a);
    // the host form's staging: v | v_blinding | states_in, then V | V_compressed | states_out, each only when asked for
    const size_t b_sc = tot * 32, b_st = a.states_in ? nv * 32 : 0, b_V = a.V ? tot * 64 : 0, b_Vc = a.V_compressed ? tot * 32 : 0;
    PoolBlock stage(ctx);
    if (!pool_alloc(ctx, &stage.p, 2 * b_sc + 2 * b_st + b_V + b_Vc)) return BPGPU_E_OOM;
    uint8_t *dv = (uint8_t *)stage.p, *dvb = dv + b_sc, *dsi = dvb + b_sc, *dV = dsi + b_st, *dVc = dV + b_V, *dso = dVc + b_Vc;
    CK(h2d(ctx, dv, a.v, b_sc));
    CK(h2d(ctx, dvb, a.v_blinding, b_sc));
    CK(h2d(ctx, dsi, a.states_in, b_st));
    CK(commit_values_locked(ctx, g, nv, m, {dv, dvb, b_st ? dsi : nullptr, b_V ? dV : nullptr, b_Vc ? dVc : nullptr, b_st ? dso : nullptr}));
    return checked_download(ctx, {{a.V, dV, b_V}, {a.V_compressed, dVc, b_Vc}, {a.states_out, dso, b_st}});
  });
}
int bpgpu_r1cs_commit_values_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const void *v, const void *v_blinding,
                                 const void *states_in, void *V, void *V_compressed, void *states_out) {
  return commit_values_entry(ctx, g, nb, 1, m, {v, v_blinding, states_in, V, V_compressed, states_out}, true);
}
int bpgpu_r1cs_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const uint8_t *v, const uint8_t *v_blinding,
                             const uint8_t *states_in, uint8_t *V, uint8_t *V_compressed, uint8_t *states_out) {
  return commit_values_entry(ctx, g, nb, 1, m, {v, v_blinding, states_in, V, V_compressed, states_out}, false);
}
int bpgpu_mpc_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const uint8_t *v, const uint8_t *v_blinding, uint8_t *V) {
  return commit_values_entry(ctx, g, nb, 3, m, {v, v_blinding, nullptr, V, nullptr, nullptr}, false);
}
/* scalars[i] * (curve generator): GeneratorsChain::next (generators.rs:112-124), Q = w * B (prover.rs:687) */
int bpgpu_generator_mul(bpgpu_ctx *ctx, const uint8_t *scalars, size_t n, uint8_t *out) {
  if (!ctx || (n && (!scalars || !out))) return BPGPU_E_ARG;
  if (!n) return BPGPU_OK;
  static const uint8_t GEN[64] = {0xca,0xcf,0x43,0xc9,0x8b,0x3d,0x72,0x3d,0xe0,0x19,0x18,0x0d,0x9b,0xfd,0xac,0xde,0xc7,0xf0,0x40,0x5a,0x41,0xed,0xec,0x7b,0x1b,0x97,0x99,0x85,0xc1,0x15,0xef,0x01,
                                  0x1f,0xdc,0xe8,0x36,0x0c,0x00,0x73,0x28,0xa3,0x43,0xbe,0x1a,0xd1,0xec,0x53,0xde,0x62,0xec,0x46,0xdf,0x01,0x48,0xbe,0xb7,0x30,0x97,0xa4,0x0a,0x06,0x68,0x56,0x00};
  bool have;
  { std::lock_guard<std::mutex> lk(ctx->mu); have = ctx->gen_tab != nullptr; }
  if (!have) {   // fixed-base table of the generator: 16 windows x 2^15 multiples (34 MB), built once per context
    bpgpu_gens *t = nullptr;
    int rc = bpgpu_gens_create(ctx, nullptr, nullptr, 0, GEN, GEN, 16, &t);   // takes the context lock itself
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->gen_tab) ctx->gen_tab = t;
    else { hipFree(t->points); hipFree(t->table); delete t; }   // another thread won the race
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  void *dsc, *dres, *dout;
  CK(ws_get(ctx, WS_ARG0, n * 32, &dsc));
  CK(ws_get(ctx, WS_ARG3, n * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG5, n * 64, &dout));
  CK(flag_reset(ctx));
  CK(h2d(ctx, dsc, scalars, n * 32));
  scalars_check(ctx->st, (Words8 *)dsc, n, ctx->d_flag);
  fixed_single16(ctx->st, ctx->gen_tab->table, (const uint32_t *)dsc, (JacRaw *)dres, n);   // 16 table additions per scalar
  jac_to_boundary(ctx->st, (JacRaw *)dres, (Words8 *)dout, n);
  return checked_download(ctx, {{out, dout, n * 64}});
}

/* ---- two-party prover: one party's local arithmetic (src/r1cs_mpc/ of the reference; include/bpgpu.h, k_mpc.hip).  A session of nb
 * proofs holds 3 nb virtual provers v = 3 p + k (k = 0 share, 1 MAC share, 2 public modifier): the linear steps are the single-party
 * launches over them, the products of two shared values go through the host's Beaver triples. ---------------------------------- */
int bpgpu_mpc_prover_commit(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover **session, size_t nb, size_t n_new, const uint8_t *a_L,
                            const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *blindings,
                            uint8_t *commitments) {
  if (!ctx || !g || !session || !nb || !blindings || !commitments) return BPGPU_E_ARG;
  if (n_new && (!a_L || !a_R || !a_O || !s_L || !s_R)) return BPGPU_E_ARG;   // blinding vectors come shared from the fabric: explicit only
  if (ctx->shard_world > 1) return BPGPU_E_ARG;
  if (*session && ((*session)->planes != 3 || (*session)->polys)) return BPGPU_E_ARG;
  if (*session && (*session)->nb != 3 * nb) return BPGPU_E_LEN;
  return prover_commit_impl(ctx, g, session, 3 * nb, n_new, a_L, a_R, a_O, s_L, s_R, nullptr, blindings, commitments, 3);
}
int bpgpu_mpc_prover_polys_mask(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                const uint8_t *gadget_challenges, const uint8_t *triples, uint8_t *masked) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !c || !y || !z || !triples || !masked || s->planes != 3) return BPGPU_E_ARG;
    if ((c->nchi != 0) != (gadget_challenges != nullptr) || ctx->shard_world > 1) return BPGPU_E_ARG;
    if (c->n != s->wn || s->polys) return BPGPU_E_LEN;     // the circuit's multipliers are the session's; one polynomial build per session
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nb = s->nb / 3, n = c->n, m = c->m, ntrip = nb * 6 * 9 * n, nmask = nb * 6 * 6 * n;
    const std::vector<uint8_t> y3 = bcast3(y, nb);
    PolysBuild build{ctx, s};
    void *dm;
    CK(ws_get(ctx, WS_MSM2, nmask * 32, &dm));
    PolyChallenges ch;
    CK(session_polys_begin(ctx, s, c, y3.data(), z, gadget_challenges, &ch));
    PoolTake M{ctx};
    M(&s->trip, ntrip * 32); M(&s->wv, nb * m * 32);
    if (!M.ok) return BPGPU_E_OOM;
    CK(h2d(ctx, s->trip, triples, ntrip * 32));
    scalars_from_ark(ctx->st, s->trip, s->trip, ntrip, ctx->d_flag);
    ProfSpan span(ctx, 17, ctx->st);
    const int32_t *dzp;
    CK(session_polys_powers(ctx, s, c, ch, &dzp));
    mpc_polys(ctx->st, circuit_dev(c), nb, s->y, s->yinv, s->aL, s->aR, s->aO, s->sL, s->sR, dzp, s->polys, s->wv, s->trip, (Words8 *)dm);
    scalars_to_ark(ctx->st, (const Words8 *)dm, (Words8 *)dm, nmask, ctx->d_flag);
    span.close();
    CK(checked_download(ctx, {{masked, dm, nmask * 32}}));
    build.kept = true;
    s->n = n; s->m = m;
    return BPGPU_OK;
  });
}
int bpgpu_mpc_prover_polys_finish(bpgpu_ctx *ctx, bpgpu_prover *s, const uint8_t *opened, const uint8_t *t_blindings, uint8_t *t_coeffs,
                                  uint8_t *T, uint8_t *wV) {
  if (!ctx || !s || !opened || !t_blindings || !t_coeffs || !T || s->planes != 3) return BPGPU_E_ARG;
  if (!s->polys || s->finished || (s->m && !wV)) return BPGPU_E_ARG;   // after bpgpu_mpc_prover_polys_mask, once
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t NB = s->nb, nb = NB / 3, n = s->n, nop = nb * 6 * 2 * n;
  void *dop, *dsc, *dres, *dout;
  CK(ws_get(ctx, WS_MSM2, nop * 32, &dop));
  CK(ws_get(ctx, WS_ARG0, NB * (5 + 6 + 10) * 32, &dsc));
  CK(ws_get(ctx, WS_ARG4, NB * 5 * sizeof(JacRaw), &dres));
  CK(ws_get(ctx, WS_ARG5, NB * 5 * 64, &dout));
  Words8 *dtb = (Words8 *)dsc, *dt = dtb + NB * 5, *rows = dt + NB * 6;
  CK(flag_reset(ctx));
  CK(h2d(ctx, dop, opened, nop * 32));
  CK(h2d(ctx, dtb, t_blindings, NB * 5 * 32));
  scalars_from_ark(ctx->st, (const Words8 *)dop, (Words8 *)dop, nop, ctx->d_flag);
  scalars_from_ark(ctx->st, dtb, dtb, NB * 5, ctx->d_flag);
  ProfSpan span(ctx, 17, ctx->st);
  mpc_tcoeffs(ctx->st, nb, n, s->polys, (const Words8 *)dop, s->trip, dt);
  mpc_t_rows(ctx->st, NB, dt, dtb, rows);
  CK(msm_gens_dev(ctx, s->g, NB * 5, 0, (const uint32_t *)rows, (JacRaw *)dres, ctx->st));   // commit_shared, mpc_prover.rs:836-856
  jac_to_boundary(ctx->st, (const JacRaw *)dres, (Words8 *)dout, NB * 5);
  scalars_to_ark(ctx->st, dt, dt, NB * 6, ctx->d_flag);
  span.close();
  CK(checked_download(ctx, {{t_coeffs, dt, NB * 6 * 32}, {T, dout, NB * 5 * 64}, {wV, s->wv, nb * s->m * 32}}));
  s->finished = true;
  return BPGPU_OK;
}
int bpgpu_mpc_prover_ipp_begin(bpgpu_ctx *ctx, bpgpu_prover *ps, const bpgpu_gens *g, size_t padded_n, size_t n1, const uint8_t *x,
                               const uint8_t *u, const uint8_t *w, bpgpu_ipp **out) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !ps || !g || !x || !u || !w || !out || ps->planes != 3 || !ps->finished || ctx->shard_world > 1) return BPGPU_E_ARG;
    const size_t nb = ps->nb / 3;
    const std::vector<uint8_t> x3 = bcast3(x, nb), u3 = bcast3(u, nb), w3 = bcast3(w, nb);
    return prover_ipp_begin_impl(ctx, ps, g, padded_n, n1, x3.data(), u3.data(), nullptr, w3.data(), out);
  });
}
int bpgpu_mpc_ipp_mask(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *triples, uint8_t *masked) {
  if (!ctx || !s || !triples || !masked || s->planes != 3) return BPGPU_E_ARG;
  if (s->n < 2) return BPGPU_E_LEN;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t nb = s->nb / 3, h = s->n / 2, ntrip = nb * 2 * 9 * h, nmask = nb * 2 * 6 * h;
  void *dm;
  CK(ws_get(ctx, WS_MSM2, nmask * 32, &dm));
  CK(flag_reset(ctx));
  CK(h2d(ctx, s->trip, triples, ntrip * 32));
  ProfSpan span(ctx, 20, ctx->st);
  scalars_from_ark(ctx->st, s->trip, s->trip, ntrip, ctx->d_flag);
  mpc_ipp_mask(ctx->st, nb, h, s->a[s->cur], s->b[s->cur], s->trip, (Words8 *)dm);
  scalars_to_ark(ctx->st, (const Words8 *)dm, (Words8 *)dm, nmask, ctx->d_flag);
  span.close();
  CK(checked_download(ctx, {{masked, dm, nmask * 32}}));
  s->masked = true;
  return BPGPU_OK;
}
int bpgpu_mpc_ipp_round(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *opened, uint8_t *L, uint8_t *R) {
  return noexcept_abi([&]() -> int {
    if (!ctx || !s || !opened || !L || !R || s->planes != 3 || !s->masked) return BPGPU_E_ARG;
    if (s->n < 2) return BPGPU_E_LEN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCK(ctx, hipSetDevice(ctx->device));
    const size_t nb = s->nb / 3, h = s->n / 2, nop = nb * 2 * 2 * h;
    void *dop;
    CK(ws_get(ctx, WS_MSM2, nop * 32, &dop));
    CK(flag_reset(ctx));
    CK(h2d(ctx, dop, opened, nop * 32));
    scalars_from_ark(ctx->st, (const Words8 *)dop, (Words8 *)dop, nop, ctx->d_flag);
    CK(checked_inputs(ctx));            // before the session state advances
    {
      ProfSpan span(ctx, 20, ctx->st);
      mpc_ipp_combine(ctx->st, nb, h, (const Words8 *)dop, s->trip, s->cLR);   // c_L, c_R per plane: mpc_inner_product.rs:142-155
      CK(ipp_round_dev(ctx, s, s->out_xy, true));
    }
    CK(download_pairs(ctx, s->out_xy, s->nb, 1, L, R));
    s->masked = false;
    return BPGPU_OK;
  });
}

#pragma GCC visibility pop
}  // extern "C"

/* ---- what bpgpu_witness.hip takes from this file (bpgpu_internal.h) ------------------------------------------------------------------ */
int bpgpu_internal_enter(bpgpu_ctx *ctx, bpgpu_internal_view *view) {
  ctx->mu.lock();
  if (hipSetDevice(ctx->device) != hipSuccess) {
    ctx->err = "hipSetDevice failed";
    ctx->mu.unlock();
    return BPGPU_E_DEVICE;
  }
  *view = {ctx->st, ctx->d_flag, ctx->opt[BPGPU_OPT_WITNESS_ROUTE], ctx->opt[BPGPU_OPT_WITNESS_SCAN_MIN], ctx->shard_world};
  return BPGPU_OK;
}
void bpgpu_internal_leave(bpgpu_ctx *ctx) { ctx->mu.unlock(); }
size_t bpgpu_internal_shard_world(bpgpu_ctx *ctx) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->shard_world;
}
void *bpgpu_internal_pool_alloc(bpgpu_ctx *ctx, size_t bytes) {
  void *p = nullptr;
  return pool_alloc(ctx, &p, bytes) ? p : nullptr;
}
void bpgpu_internal_pool_release(bpgpu_ctx *ctx, void *p) { pool_release(ctx, p); }
int bpgpu_internal_hip(bpgpu_ctx *ctx, hipError_t e, const char *what) {
  if (e == hipSuccess) return BPGPU_OK;
  ctx->err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? BPGPU_E_OOM : BPGPU_E_DEVICE;
}
void bpgpu_internal_prof_mark(bpgpu_ctx *ctx, int kind) { if (ctx->prof) ProfScope::mark(ctx, kind, ctx->st); }
int bpgpu_internal_flag_reset(bpgpu_ctx *ctx) { return flag_reset(ctx); }
int bpgpu_internal_checked_wait(bpgpu_ctx *ctx) { return checked_download(ctx, {}); }
void bpgpu_internal_circuit_dims(const bpgpu_circuit *c, size_t *n, size_t *m, size_t *nchi) { *n = c->n; *m = c->m; *nchi = c->nchi; }
// a two-phase prover's circuit and label: a numeric circuit has no gadget challenge (bpgpu_r1cs_prove_fs); with labels attached the
// call's label must be null; without, one label per schedule (required only where the call has work: need_label)
int bpgpu_internal_prove_fs2_labels(const bpgpu_circuit *c, const uint8_t *gadget_label, bool need_label) {
  if (!c->nchi) return BPGPU_E_ARG;
  return gadget_label_rule(c, gadget_label, c->nchi == 1 && (gadget_label || !need_label));
}
int bpgpu_internal_prove_fs2_shape(const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1) {
  if (!c->nchi) return BPGPU_E_ARG;
  if (!nb) return BPGPU_OK;
  if (n1 >= c->n) return BPGPU_E_LEN;
  if (prove_fs_dims(c).padded_n > g->cap) return BPGPU_E_GENS;
  return BPGPU_OK;
}
int bpgpu_internal_prove_fs2_chains(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                    const bpgpu_internal_fs2 &io, int (*between)(void *user, const void *chi_dev), void *user) {
  ProverOwner own(nullptr, ProverFree{ctx});   // the session of the call: its buffers go back to the pool on the way out, whatever the outcome
  CK(prove_fs2_begin_locked(ctx, g, c, nb, n1, {io.states_in, io.gadget_label, io.a_L1, io.a_R1, io.a_O1, io.s_L1, io.s_R1, io.keys1, io.blindings1,
                                                nullptr, io.gadget_challenges_out, nullptr}, own));
  CK(between(user, fs2_arrays(own.get()).chi));
  return prove_fs2_finish_locked(ctx, g, c, own, {nullptr, io.a_L2, io.a_R2, io.a_O2, io.s_L2, io.s_R2, io.keys2, io.v_blinding, io.blindings2,
                                                  io.proof_points, io.proof_scalars, io.wire, io.challenges_out, io.states_out});
}
// the stages of bpgpu_r1cs_prove_values: the _locked functions of the entry points above, as they stand
int bpgpu_internal_prove_fs_shape(const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb) {
  if (c->nchi) return BPGPU_E_ARG;       // a two-phase prover evaluates its gadget on the challenge: bpgpu_r1cs_prove_fs2
  if (!nb) return BPGPU_OK;
  if (!c->n) return BPGPU_E_LEN;         // (no multipliers: no IPP to speak of; the staged calls serve such circuits)
  return prove_fs_dims(c).padded_n > g->cap ? BPGPU_E_GENS : BPGPU_OK;
}
int bpgpu_internal_commit_values_shape(size_t nb, size_t m) {
  return nb > COMMIT_VALUES_MAX || (m && nb > COMMIT_VALUES_MAX / m) ? BPGPU_E_LEN : BPGPU_OK;
}
int bpgpu_internal_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const void *v, const void *v_blinding,
                                 const void *states_in, void *V, void *V_compressed, void *states_out) {
  return commit_values_locked(ctx, g, nb, m, {v, v_blinding, states_in, V, V_compressed, states_out});
}
int bpgpu_internal_rows_fit(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb) {
  RowsDev view;
  CK(circuit_view(ctx, c, &view));
  return rows_eval_fits(view, nb) ? BPGPU_OK : BPGPU_E_LEN;
}
int bpgpu_internal_constraints_satisfied(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const void *a_L, const void *a_R, const void *a_O,
                                         const void *v, const void *gadget_challenges, void *ok, void *first_bad_row, void *first_bad_gate) {
  return rows_locked(ctx, c, nb, 1, {a_L, a_R, a_O, v, gadget_challenges, ok, first_bad_row, first_bad_gate, nullptr}, true);
}
int bpgpu_internal_prove_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const bpgpu_internal_fs1 &io) {
  return prove_fs_locked(ctx, g, c, nb, {io.states_in, io.a_L, io.a_R, io.a_O, io.s_L, io.s_R, io.vector_keys, io.v_blinding, io.blindings,
                                         io.proof_points, io.proof_scalars, io.wire, io.challenges_out, io.states_out});
}

