// bpgpu_mpc_witness.hip -- the two-party prover's witness synthesis of include/bpgpu.h (bpgpu_mpc_witness_*): a session that walks the
// dependency levels of a bpgpu_witness program, one _mask / _combine pair -- one opening -- per level, on top of k_mpc_witness.hip;
// and bpgpu_witness_gate_levels, which tells a host which gate each triple of a round belongs to.  Host forms only, like every
// bpgpu_mpc_* call.  The program handle and the scaffolding of an entry point are witness_host.h's.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/bpgpu.h"
#include "witness_host.h"

using namespace bpk;

// (the leading fields are what the refusals on the order of the calls read)
struct bpgpu_mpc_witness {
  size_t nb = 0;
  uint32_t left = 0, len = 0;   // levels still to run | gates of the next one (0: none left)
  uint32_t masked = 0;          // a _mask awaits its _combine
  const bpgpu_witness *w = nullptr;
  uint32_t level = 0;           // the next level in the program's numbering (phase 1's levels first)
  size_t widest = 0;            // gates of the session's widest level: what trip and io are sized for
  // one pool allocation, plain canonical words: the planes 3 nb x n, v 3 nb x m, the input pairs 3 nb x ninp x 2, chi nb x nchi, the
  // current level's triples 9 nb x widest, and the staging of masked (6 nb x widest) / opened (2 nb x widest)
  Words8 *mem = nullptr, *L = nullptr, *R = nullptr, *O = nullptr, *v = nullptr, *in = nullptr, *chi = nullptr, *trip = nullptr, *io = nullptr;
  bool has_chi = false;
};

namespace {

constexpr size_t MPC_WIT_MAX = (size_t)1 << 30;     // 3 nb n and 3 nb m: the launches index with room to spare below that

void next_level(bpgpu_mpc_witness *s) {
  s->len = s->left ? s->w->level_ptr[s->level + 1] - s->w->level_ptr[s->level] : 0;
}
MpcWitLevel level_args(const bpgpu_mpc_witness *s) {
  const bpgpu_witness *w = s->w;
  return {w->dev, s->nb, w->level_ptr[s->level], w->level_long[s->level], w->level_ptr[s->level + 1], s->L, s->R, s->O, s->v, s->in,
          s->has_chi ? s->chi : nullptr, s->trip, s->io};
}
// `count` ark scalars from the host into dst as plain canonical words (a non-canonical one raises the flag)
int ark_in(const Entered &e, Words8 *dst, const uint8_t *src, size_t count) {
  if (!count) return BPGPU_OK;
  WHIP(e.ctx, hipMemcpyAsync(dst, src, count * 32, hipMemcpyHostToDevice, e.view.st));
  witness_convert(e.view.st, false, 1, count, dst, count, dst, count, e.view.d_flag);
  return BPGPU_OK;
}

int begin_check(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const void *v, const void *inputs, const void *chi, const void *aL,
                const void *aR, const void *aO, bpgpu_mpc_witness **out) {
  if (!ctx || !w || !out || phase < 0 || phase > 2) return BPGPU_E_ARG;
  const bool want_chi = w->nchi != 0 && phase != 1;
  if (want_chi != (chi != nullptr)) return BPGPU_E_ARG;
  if ((phase != 2 && w->bits[0]) || (phase != 1 && w->bits[1])) return BPGPU_E_ARG;   // a bit of a shared value is not a local function
  if ((phase != 2 && w->invs[0]) || (phase != 1 && w->invs[1])) return BPGPU_E_ARG;   // ... and neither is its inverse
  if ((phase != 2 && w->divs[0]) || (phase != 1 && w->divs[1])) return BPGPU_E_ARG;   // ... nor its integer quotient
  if (bpgpu_internal_shard_world(ctx) > 1) return BPGPU_E_ARG;
  if (!nb) return BPGPU_OK;
  if ((w->m && !v) || (w->ninp && !inputs)) return BPGPU_E_ARG;
  if (phase == 2 && w->n && (!aL || !aR || !aO)) return BPGPU_E_ARG;
  const size_t widest = std::max(w->n, w->m);
  if (nb > MPC_WIT_MAX / 3 || (widest && 3 * nb > MPC_WIT_MAX / widest)) return BPGPU_E_LEN;
  return BPGPU_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int bpgpu_witness_gate_levels(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                              const uint32_t *idx, uint32_t *level) {
  return no_throw([&]() -> int {
    if (n && !level) return BPGPU_E_ARG;
    return bpgpu_internal_witness_levels(n, n1, nchi, op, row_ptr, kind, idx, level);
  });
}

int bpgpu_mpc_witness_begin(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const uint8_t *v, const uint8_t *inputs,
                            const uint8_t *gadget_challenges, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                            bpgpu_mpc_witness **out) {
  return no_throw([&]() -> int {
    if (out) *out = nullptr;
    WCK(begin_check(ctx, w, nb, phase, v, inputs, gadget_challenges, a_L, a_R, a_O, out));
    if (!nb) return BPGPU_OK;
    bpgpu_mpc_witness *s = new (std::nothrow) bpgpu_mpc_witness();
    if (!s) return BPGPU_E_OOM;
    s->nb = nb; s->w = w;
    s->level = phase == 2 ? w->levels[0] : 0;
    s->left = (phase == 2 ? 0 : w->levels[0]) + (phase == 1 ? 0 : w->levels[1]);
    for (uint32_t l = s->level; l < s->level + s->left; l++) s->widest = std::max<size_t>(s->widest, w->level_ptr[l + 1] - w->level_ptr[l]);
    next_level(s);
    s->has_chi = gadget_challenges != nullptr;
    Entered e(ctx);
    int rc = e.enter();
    if (rc != BPGPU_OK) { delete s; return rc; }
    const size_t nv = 3 * nb, plane = nv * w->n, c_v = nv * w->m, c_in = nv * 2 * w->ninp, c_chi = s->has_chi ? nb * w->nchi : 0;
    s->mem = (Words8 *)bpgpu_internal_pool_alloc(ctx, (3 * plane + c_v + c_in + c_chi + 15 * nb * s->widest + 1) * 32);
    if (!s->mem) { delete s; return BPGPU_E_OOM; }
    s->L = s->mem; s->R = s->L + plane; s->O = s->R + plane; s->v = s->O + plane; s->in = s->v + c_v; s->chi = s->in + c_in;
    s->trip = s->chi + c_chi; s->io = s->trip + 9 * nb * s->widest;
    hipStream_t st = e.view.st;
    rc = [&]() -> int {
      Prof22 prof(ctx);
      WCK(bpgpu_internal_flag_reset(ctx));
      if (plane) WHIP(ctx, hipMemsetAsync(s->L, 0, 3 * plane * 32, st));      // a multiplier never given is zero
      WCK(ark_in(e, s->v, v, c_v));
      WCK(ark_in(e, s->in, inputs, c_in));
      if (c_chi) {
        WHIP(ctx, hipMemcpyAsync(s->chi, gadget_challenges, c_chi * 32, hipMemcpyHostToDevice, st));
        scalars_check(st, s->chi, c_chi, e.view.d_flag);
      }
      if (phase == 2 && w->n1) {         // phase 1 as the caller holds it: the first n1 multipliers of every plane
        const uint8_t *src[3] = {a_L, a_R, a_O};
        Words8 *dst[3] = {s->L, s->R, s->O};
        for (int k = 0; k < 3; k++) {
          WHIP(ctx, hipMemcpy2DAsync(dst[k], w->n * 32, src[k], w->n * 32, w->n1 * 32, nv, hipMemcpyHostToDevice, st));
          witness_convert(st, false, nv, w->n1, dst[k], w->n, dst[k], w->n, e.view.d_flag);
        }
      }
      return bpgpu_internal_checked_wait(ctx);
    }();
    if (rc != BPGPU_OK) { bpgpu_internal_pool_release(ctx, s->mem); delete s; return rc; }
    *out = s;
    return BPGPU_OK;
  });
}

size_t bpgpu_mpc_witness_levels_left(const bpgpu_mpc_witness *s) { return s ? s->left : 0; }
size_t bpgpu_mpc_witness_level_len(const bpgpu_mpc_witness *s) { return s ? s->len : 0; }

int bpgpu_mpc_witness_mask(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, const uint8_t *triples, uint8_t *masked) {
  return no_throw([&]() -> int {
    if (!ctx || !s || !triples || !masked || s->masked || !s->left) return BPGPU_E_ARG;
    Entered e(ctx);
    WCK(e.enter());
    const size_t G = s->len;
    WCK(bpgpu_internal_flag_reset(ctx));
    {
      Prof22 prof(ctx);
      WCK(ark_in(e, s->trip, triples, 9 * s->nb * G));
      mpc_witness_mask(e.view.st, level_args(s));
      witness_convert(e.view.st, true, 1, 6 * s->nb * G, s->io, 0, s->io, 0, e.view.d_flag);
    }
    WCK(bpgpu_internal_checked_wait(ctx));
    WHIP(ctx, hipMemcpyAsync(masked, s->io, 6 * s->nb * G * 32, hipMemcpyDeviceToHost, e.view.st));
    WHIP(ctx, hipStreamSynchronize(e.view.st));
    s->masked = 1;
    return BPGPU_OK;
  });
}

int bpgpu_mpc_witness_combine(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, const uint8_t *opened) {
  return no_throw([&]() -> int {
    if (!ctx || !s || !opened || !s->masked) return BPGPU_E_ARG;
    Entered e(ctx);
    WCK(e.enter());
    WCK(bpgpu_internal_flag_reset(ctx));
    {
      Prof22 prof(ctx);
      WCK(ark_in(e, s->io, opened, 2 * s->nb * s->len));
      mpc_witness_combine(e.view.st, level_args(s), s->io);
    }
    WCK(bpgpu_internal_checked_wait(ctx));       // (a refused `opened` leaves the level masked: the call may be repeated)
    s->masked = 0;
    s->level++;
    s->left--;
    next_level(s);
    return BPGPU_OK;
  });
}

int bpgpu_mpc_witness_finish(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, uint8_t *a_L, uint8_t *a_R, uint8_t *a_O) {
  return no_throw([&]() -> int {
    if (!ctx || !s || s->left || s->masked) return BPGPU_E_ARG;
    const size_t plane = 3 * s->nb * s->w->n;
    if (plane && (!a_L || !a_R || !a_O)) return BPGPU_E_ARG;
    if (!plane) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    Scratch sc(ctx);
    Words8 *stage = (Words8 *)sc.take(3 * plane * 32);       // (the session's planes stay plain: the call may be repeated)
    if (!stage) return BPGPU_E_OOM;
    WCK(bpgpu_internal_flag_reset(ctx));
    {
      Prof22 prof(ctx);
      witness_convert(e.view.st, true, 1, 3 * plane, s->L, 0, stage, 0, e.view.d_flag);
    }
    WCK(bpgpu_internal_checked_wait(ctx));
    uint8_t *host[3] = {a_L, a_R, a_O};
    for (int k = 0; k < 3; k++) WHIP(ctx, hipMemcpyAsync(host[k], stage + k * plane, plane * 32, hipMemcpyDeviceToHost, e.view.st));
    WHIP(ctx, hipStreamSynchronize(e.view.st));
    return BPGPU_OK;
  });
}

void bpgpu_mpc_witness_destroy(bpgpu_ctx *ctx, bpgpu_mpc_witness *s) {
  if (!s) return;
  if (ctx && s->mem) {
    Entered e(ctx);
    if (e.enter() == BPGPU_OK) bpgpu_internal_pool_release(ctx, s->mem);
  }
  delete s;
}

#pragma GCC visibility pop
}  // extern "C"
