// witness_host.h -- what the two host files of the witness synthesis share (bpgpu_witness.hip: gate programs and the single-party
// entry points; bpgpu_mpc_witness.hip: the two-party sessions): the program handle and the scaffolding of an entry point.  Not exported.
#ifndef BPGPU_WITNESS_HOST_H
#define BPGPU_WITNESS_HOST_H
#include <new>
#include <vector>

#include "bpgpu_internal.h"
#include "kernels.h"

// (the leading fields are what the refusals on arguments read)
struct bpgpu_witness {
  size_t n = 0, n1 = 0, m = 0, nchi = 0, ninp = 0;
  uint32_t bits[2] = {0, 0};    // BIT gates per phase
  uint32_t invs[2] = {0, 0};    // INV gates per phase
  uint32_t divs[2] = {0, 0};    // DIVREM gates per phase
  uint32_t levels[2] = {0, 0};
  // per phase: the extended compressed levels (the scan lists are the extended chains'; without an affine member those are the
  // product chains'), the longest product chain, the longest extended chain, and whether the phase has an affine member
  uint32_t scan_levels[2] = {0, 0}, longest[2] = {0, 0}, xlongest[2] = {0, 0};
  bool affine[2] = {false, false};
  void *mem = nullptr;          // one device allocation: everything dev points to
  bpk::WitDev dev{};
  std::vector<uint32_t> level_ptr, level_long;   // host copies of dev's: the two-party sessions walk the levels from the host
};

// per-gate dependency levels of a program, each within its phase, from the shape analysis of bpgpu_witness_plan (its refusals)
BPGPU_HIDDEN int bpgpu_internal_witness_levels(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr,
                                               const uint32_t *kind, const uint32_t *idx, uint32_t *level);

#define WCK(x) do { int rc__ = (x); if (rc__ != BPGPU_OK) return rc__; } while (0)
#define WHIP(ctx, call) WCK(bpgpu_internal_hip(ctx, (call), #call))

namespace {
// the context's mutex for the length of an entry point
struct Entered {
  bpgpu_ctx *ctx;
  bool in = false;
  bpgpu_internal_view view{};
  explicit Entered(bpgpu_ctx *c) : ctx(c) {}
  int enter() { const int rc = bpgpu_internal_enter(ctx, &view); in = rc == BPGPU_OK; return rc; }
  ~Entered() { if (in) bpgpu_internal_leave(ctx); }
};
// pool buffers of a call, given back on the way out (stream-ordered reuse); declared AFTER the Entered of its call: released under the mutex
struct Scratch {
  bpgpu_ctx *ctx;
  std::vector<void *> held;
  explicit Scratch(bpgpu_ctx *c) : ctx(c) { held.reserve(8); }
  void *take(size_t bytes) {
    void *p = bpgpu_internal_pool_alloc(ctx, bytes);
    if (p) held.push_back(p);
    return p;
  }
  ~Scratch() { for (void *p : held) bpgpu_internal_pool_release(ctx, p); }
};
struct Prof22 {   // kind 22: the launches only the one-call chains have
  bpgpu_ctx *ctx;
  explicit Prof22(bpgpu_ctx *c) : ctx(c) { bpgpu_internal_prof_mark(ctx, 22); }
  ~Prof22() { bpgpu_internal_prof_mark(ctx, 22); }
};
template <class Body> int no_throw(Body body) {
  try { return body(); } catch (const std::bad_alloc &) { return BPGPU_E_OOM; }
}
}  // namespace
#endif
