// bpgpu_witness.hip -- the witness-synthesis entry points of include/bpgpu.h: gate programs (bpgpu_witness_create / _plan), their
// evaluation (bpgpu_r1cs_witness_synthesize), the one-call two-phase prover (bpgpu_r1cs_prove_fs2) on top of k_witness.hip, and the
// call that chains commitments, synthesis, check and proof from the provers' values (bpgpu_r1cs_prove_values).  The context, its
// pool and the provers' chains live in bpgpu_api.hip; what this file takes from there is in bpgpu_internal.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/bpgpu.h"
#include "witness_host.h"       // struct bpgpu_witness, the scaffolding of an entry point
#include "witness_dev.cuh"

using namespace bpk;
using namespace bp;

static_assert(BPGPU_GATE_MUL == WIT_OP_MUL && BPGPU_GATE_INPUT == WIT_OP_INPUT && BPGPU_GATE_BIT == WIT_OP_BIT &&
              BPGPU_GATE_INV == WIT_OP_INV && BPGPU_GATE_DIVREM == WIT_OP_DIVREM, "gate ops of the header");

namespace {

// The route of a phase.  Both forms are bound by the latency of one dependent gate after the other (about 10 us each, measured): a
// lane pays it once per GATE, a block once per LEVEL, so the block form wins as soon as a level holds two gates -- profiles/
// witness_synth.log: 0.74 against 1.22 ms for 256 shuffles of 63 levels x 2 gates, 0.074 against 7.4 ms for 256 range programs of one
// level x 1024, 171 against 352 ms for one chain pair of 16 383 levels x 2 (DESIGN.md "Witness synthesis").  Those runs have at most
// 256 provers, where every block is resident at once.  Beyond WIT_BLOCKS_RESIDENT provers the blocks run in rounds, and the width
// asked for grows with the rounds: an extrapolation, not a measurement.
constexpr size_t WIT_BLOCK_MIN_WIDTH = 2, WIT_BLOCKS_RESIDENT = 1024;
int wit_route(size_t gates, uint32_t levels, size_t nb) {
  if (!gates) return 0;
  const size_t rounds = (nb + WIT_BLOCKS_RESIDENT - 1) / WIT_BLOCKS_RESIDENT;
  if (rounds > gates) return 1;      // (also keeps the product below in range)
  return gates >= WIT_BLOCK_MIN_WIDTH * (rounds ? rounds : 1) * levels ? 2 : 1;
}

// The scan form (bpgpu.h "product chains"): from how many members of a phase's longest chain it is taken when nothing is forced.
// WIT_SCAN_MIN_DEFAULT (bpgpu_internal.h) is read from the sweep of profiles/witness_synth.log.
// A phase's longest EXTENDED chain (xlongest: product and affine members) takes it from max(scan_min, WIT_AFFINE_MIN) members on,
// read from profiles/witness_affine.log -- except that scan_min == 1 keeps its meaning "every chain", of either kind.
int wit_route_scan(size_t gates, uint32_t levels, uint32_t longest, uint32_t xlongest, size_t nb, int64_t scan_min) {
  if (gates && scan_min > 0) {
    if ((int64_t)longest >= scan_min) return 3;
    if ((int64_t)xlongest >= (scan_min == 1 ? 1 : std::max(scan_min, WIT_AFFINE_MIN))) return 3;
  }
  return wit_route(gates, levels, nb);
}

constexpr uint32_t WIT_NONE = 0xFFFFFFFFu;
struct WitShape {
  std::vector<uint32_t> level;    // per gate, within its phase
  std::vector<uint32_t> row_len;  // per row 2 i, 2 i + 1: the terms of all 1 + nchi blocks
  uint32_t levels[2] = {0, 0}, widest = 0, nlong = 0, ninp = 0, ninv[2] = {0, 0}, ndiv[2] = {0, 0};
  size_t nnz = 0;
  // product chains: a member's predecessor (WIT_NONE: an ordinary gate), the side of its link row, a gate's member successor, and
  // the compressed levels, in which a member takes its predecessor's
  std::vector<uint32_t> pred, succ, scan_level;
  std::vector<uint8_t> link_right;
  uint32_t scan_levels[2] = {0, 0}, chains[2] = {0, 0}, members[2] = {0, 0}, longest[2] = {0, 0};
  // the EXTENDED chains (pass 2): the same, with the affine members among the members; is_affine: a member that pass 2 added
  std::vector<uint32_t> xpred, xsucc, xscan_level;
  std::vector<uint8_t> xlink_right, is_affine;
  uint32_t xscan_levels[2] = {0, 0}, xchains[2] = {0, 0}, xmembers[2] = {0, 0}, xaffine[2] = {0, 0}, xlongest[2] = {0, 0};
};
// Is row `side` of gate i an AFFINE link row -- exactly one stored term over all blocks of kind 0..2 on a gate of the phase, that
// term of kind 2 on a gate without a member successor of either kind yet, whatever else the row holds -- and the other row free of
// the phase's multipliers?  -> the gate linked to, or WIT_NONE
uint32_t wit_affine_link_of(size_t i, size_t side, size_t phase_lo, size_t n, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                            const uint32_t *idx, const WitShape &s) {
  const size_t rows = 2 * n;
  uint32_t j = WIT_NONE;
  for (size_t b = 0; b <= nchi; b++) {
    const size_t r = b * rows + 2 * i + side, f = b * rows + 2 * i + (1 - side);
    for (uint32_t t = row_ptr[r]; t < row_ptr[r + 1]; t++) {
      if (kind[t] > 2 || idx[t] < phase_lo) continue;
      if (kind[t] != 2 || j != WIT_NONE) return WIT_NONE;     // a link through a_L / a_R, or a second term on the phase
      j = idx[t];
    }
    for (uint32_t t = row_ptr[f]; t < row_ptr[f + 1]; t++)
      if (kind[t] <= 2 && idx[t] >= phase_lo) return WIT_NONE;
  }
  return j != WIT_NONE && s.xsucc[j] == WIT_NONE ? j : WIT_NONE;
}
// Is row `side` of gate i a link row -- one stored term over all blocks, of kind 2, on a gate of the phase that has no member
// successor yet -- and the other row free of the phase's multipliers?  -> the gate linked to, or WIT_NONE
uint32_t wit_link_of(size_t i, size_t side, size_t phase_lo, size_t n, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                     const uint32_t *idx, const WitShape &s) {
  if (s.row_len[2 * i + side] != 1) return WIT_NONE;
  const size_t rows = 2 * n;
  uint32_t j = WIT_NONE;
  for (size_t b = 0; b <= nchi; b++) {
    const size_t r = b * rows + 2 * i + side, f = b * rows + 2 * i + (1 - side);
    if (row_ptr[r + 1] > row_ptr[r]) {
      const uint32_t t = row_ptr[r];
      if (kind[t] != 2 || idx[t] < phase_lo) return WIT_NONE;
      j = idx[t];
    }
    for (uint32_t t = row_ptr[f]; t < row_ptr[f + 1]; t++)
      if (kind[t] <= 2 && idx[t] >= phase_lo) return WIT_NONE;
  }
  return j != WIT_NONE && s.succ[j] == WIT_NONE ? j : WIT_NONE;
}
// what bpgpu_witness_plan, bpgpu_witness_chains, bpgpu_witness_affine_chains and bpgpu_witness_create share: the checks that make the
// levels well defined, the levels, the product chains with the compressed levels (pass 1) and the extended chains with theirs (pass 2)
// -- all from the shape alone: no coefficient is read
int wit_analyse(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                WitShape *s) {
  if (!row_ptr || (n && !op) || n1 > n || nchi > 8) return BPGPU_E_ARG;
  if (n > ROWS_IDX_MASK) return BPGPU_E_LEN;
  const size_t rows = 2 * n, stored = (1 + nchi) * rows;
  for (size_t r = 0; r < stored; r++) if (row_ptr[r + 1] < row_ptr[r]) return BPGPU_E_ARG;
  s->nnz = row_ptr[stored];
  if (s->nnz >= 0xFFFFFF00u) return BPGPU_E_LEN;        // (a wave's lane-strided term index t + 64 must not wrap)
  if (s->nnz && (!kind || !idx)) return BPGPU_E_ARG;
  s->level.assign(n, 0);
  s->row_len.assign(rows, 0);
  s->pred.assign(n, WIT_NONE);
  s->succ.assign(n, WIT_NONE);
  s->scan_level.assign(n, 0);
  s->link_right.assign(n, 0);
  std::vector<uint32_t> width, length(n, 0);   // length: of a head, the members of its chain; of a member, its head
  for (size_t i = 0; i < n; i++) {
    if (op[i] > BPGPU_GATE_DIVREM || op[i] == 3 || op[i] == 5) return BPGPU_E_ARG;      // (3 and 5 are no ops: bpgpu.h)
    if (op[i] == BPGPU_GATE_INPUT) s->ninp++;
    if (op[i] == BPGPU_GATE_INV) s->ninv[i < n1 ? 0 : 1]++;
    if (op[i] == BPGPU_GATE_DIVREM) s->ndiv[i < n1 ? 0 : 1]++;
    const size_t phase_lo = i < n1 ? 0 : n1;
    uint32_t lvl = 0, slvl = 0;
    for (size_t side = 0; side < 2; side++)
      for (size_t j = 0; j <= nchi; j++) {
        const size_t r = j * rows + 2 * i + side;
        s->row_len[2 * i + side] += row_ptr[r + 1] - row_ptr[r];
        for (uint32_t t = row_ptr[r]; t < row_ptr[r + 1]; t++) {
          if (kind[t] > 4) return BPGPU_E_ARG;
          if (kind[t] > 2) continue;
          if (idx[t] >= i) return BPGPU_E_ARG;            // a self or forward reference
          if (idx[t] >= phase_lo && op[i] != BPGPU_GATE_INPUT) {
            lvl = std::max(lvl, s->level[idx[t]] + 1);
            slvl = std::max(slvl, s->scan_level[idx[t]] + 1);
          }
        }
      }
    s->level[i] = lvl;
    const int ph = i < n1 ? 0 : 1;
    for (size_t side = 0; side < 2 && op[i] == BPGPU_GATE_MUL && s->pred[i] == WIT_NONE; side++) {     // the left row first
      const uint32_t j = wit_link_of(i, side, phase_lo, n, nchi, row_ptr, kind, idx, *s);
      if (j == WIT_NONE) continue;
      s->pred[i] = j;
      s->succ[j] = (uint32_t)i;
      s->link_right[i] = (uint8_t)side;
      const uint32_t head = s->pred[j] == WIT_NONE ? j : length[j];
      length[i] = head;
      if (head == j) s->chains[ph]++;
      s->members[ph]++;
      s->longest[ph] = std::max(s->longest[ph], ++length[head]);
      slvl = s->scan_level[j];
    }
    s->scan_level[i] = slvl;
    s->scan_levels[ph] = std::max(s->scan_levels[ph], slvl + 1);
    if (i == n1) width.clear();
    if (width.size() <= lvl) width.resize(lvl + 1, 0);
    s->widest = std::max(s->widest, ++width[lvl]);
    s->levels[i < n1 ? 0 : 1] = (uint32_t)width.size();
  }
  // pass 2, in program order, once every product member is known (a product gate keeps its a_O whatever the order): the MUL gates
  // without a predecessor that are affine members, and with them the extended chains and their compressed levels
  s->xpred = s->pred;
  s->xsucc = s->succ;
  s->xlink_right = s->link_right;
  s->xscan_level.assign(n, 0);
  s->is_affine.assign(n, 0);
  length.assign(n, 0);
  for (size_t i = 0; i < n; i++) {
    const size_t phase_lo = i < n1 ? 0 : n1;
    const int ph = i < n1 ? 0 : 1;
    for (size_t side = 0; side < 2 && op[i] == BPGPU_GATE_MUL && s->xpred[i] == WIT_NONE; side++) {      // the left row first
      const uint32_t j = wit_affine_link_of(i, side, phase_lo, n, nchi, row_ptr, kind, idx, *s);
      if (j == WIT_NONE) continue;
      s->xpred[i] = j;
      s->xsucc[j] = (uint32_t)i;
      s->xlink_right[i] = (uint8_t)side;
      s->is_affine[i] = 1;
      s->xaffine[ph]++;
    }
    uint32_t slvl = 0;
    if (s->xpred[i] != WIT_NONE) {
      const uint32_t j = s->xpred[i], head = s->xpred[j] == WIT_NONE ? j : length[j];
      length[i] = head;
      if (head == j) s->xchains[ph]++;
      s->xmembers[ph]++;
      s->xlongest[ph] = std::max(s->xlongest[ph], ++length[head]);
      slvl = s->xscan_level[j];
    } else if (op[i] != BPGPU_GATE_INPUT) {
      for (size_t r = 2 * i; r < 2 * i + 2; r++)
        for (size_t b = 0; b <= nchi; b++)
          for (uint32_t t = row_ptr[b * rows + r]; t < row_ptr[b * rows + r + 1]; t++)
            if (kind[t] <= 2 && idx[t] >= phase_lo) slvl = std::max(slvl, s->xscan_level[idx[t]] + 1);
    }
    s->xscan_level[i] = slvl;
    s->xscan_levels[ph] = std::max(s->xscan_levels[ph], slvl + 1);
  }
  const uint32_t lane_max = rows_lane_max();
  for (uint32_t len : s->row_len) if (len > lane_max) s->nlong++;
  return BPGPU_OK;
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// the grids of k_witness.hip are addressable
bool wit_fits(const bpgpu_witness *w, size_t nb) {
  const size_t widest = std::max(std::max(w->n, w->m), 2 * w->ninp);
  return nb < ((size_t)1 << 31) && (!widest || nb <= ((size_t)1 << 38) / widest);
}

// The scratch of a run: plain canonical planes nb x n, the values, the input pairs, the challenges
struct WitRun { Words8 *L, *R, *O, *v, *in, *chi; };
int wit_begin(const Entered &e, const bpgpu_witness *w, size_t nb, const void *v, const void *inputs, Scratch &sc, WitRun *run) {
  const size_t plane = nb * w->n;
  Words8 *base = (Words8 *)sc.take((3 * plane + nb * w->m + 2 * nb * w->ninp + nb * w->nchi) * 32);
  if (!base) return BPGPU_E_OOM;
  *run = {base, base + plane, base + 2 * plane, base + 3 * plane, base + 3 * plane + nb * w->m, base + 3 * plane + nb * w->m + 2 * nb * w->ninp};
  Prof22 prof(e.ctx);
  witness_convert(e.view.st, false, nb, w->m, (const Words8 *)v, w->m, run->v, w->m, e.view.d_flag);
  witness_convert(e.view.st, false, nb, 2 * w->ninp, (const Words8 *)inputs, 2 * w->ninp, run->in, 2 * w->ninp, e.view.d_flag);
  return BPGPU_OK;
}
// one launch: the gates of phase ph (1 or 2) on the run's planes; chi: nb x nchi plain words, or nullptr for phase 1
void wit_phase(const Entered &e, const bpgpu_witness *w, size_t nb, int ph, const WitRun &run, const Words8 *chi) {
  const uint32_t n1 = (uint32_t)w->n1, n = (uint32_t)w->n;
  const uint32_t g_lo = ph == 1 ? 0 : n1, g_hi = ph == 1 ? n1 : n;
  const int route = e.view.witness_route ? (int)e.view.witness_route
                                         : wit_route_scan(g_hi - g_lo, w->levels[ph - 1], w->longest[ph - 1], w->xlongest[ph - 1], nb,
                                                          e.view.witness_scan_min);
  const uint32_t *levels = route == 3 ? w->scan_levels : w->levels;       // the scan form walks the compressed levels
  const uint32_t l_lo = ph == 1 ? 0 : levels[0];
  const int form = route == 3 && w->affine[ph - 1] ? 4 : route;           // a phase with an affine member: the affine instantiation
  Prof22 prof(e.ctx);
  witness_eval(e.view.st, w->dev, nb, form, w->invs[ph - 1] != 0, w->divs[ph - 1] != 0, g_lo, g_hi, l_lo, l_lo + levels[ph - 1], run.L, run.R, run.O, run.v, run.in, chi);
}
// the gates [lo, lo + count) of every prover, out of the run's planes into ark planes of `stride` scalars per prover
void wit_export(const Entered &e, const bpgpu_witness *w, size_t nb, const WitRun &run, size_t lo, size_t count, void *aL, void *aR, void *aO,
                size_t stride) {
  Prof22 prof(e.ctx);
  const Words8 *src[3] = {run.L, run.R, run.O};
  void *dst[3] = {aL, aR, aO};
  for (int k = 0; k < 3; k++) witness_convert(e.view.st, true, nb, count, src[k] + lo, w->n, (Words8 *)dst[k], stride, e.view.d_flag);
}

// ---- bpgpu_r1cs_witness_synthesize ----
int synth_check(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const void *v, const void *inputs, const void *chi, const void *aL,
                const void *aR, const void *aO) {
  if (!ctx || !w || phase < 0 || phase > 2) return BPGPU_E_ARG;
  const bool want_chi = w->nchi != 0 && phase != 1;
  if (want_chi != (chi != nullptr)) return BPGPU_E_ARG;
  if (!nb) return BPGPU_OK;
  if ((w->n && (!aL || !aR || !aO)) || (w->m && !v) || (w->ninp && !inputs)) return BPGPU_E_ARG;
  return wit_fits(w, nb) ? BPGPU_OK : BPGPU_E_LEN;
}
// mutex held, arguments checked, nb > 0; every pointer HBM; asynchronous
int synth_locked(const Entered &e, const bpgpu_witness *w, size_t nb, int phase, const void *v, const void *inputs, const void *chi, void *aL,
                 void *aR, void *aO) {
  Scratch sc(e.ctx);
  WitRun run;
  WCK(wit_begin(e, w, nb, v, inputs, sc, &run));
  if (chi) {
    WHIP(e.ctx, hipMemcpyAsync(run.chi, chi, nb * w->nchi * 32, hipMemcpyDeviceToDevice, e.view.st));
    scalars_check(e.view.st, run.chi, nb * w->nchi, e.view.d_flag);
  }
  if (phase == 2) {          // phase 1 as the caller holds it
    Prof22 prof(e.ctx);
    const void *src[3] = {aL, aR, aO};
    Words8 *dst[3] = {run.L, run.R, run.O};
    for (int k = 0; k < 3; k++) witness_convert(e.view.st, false, nb, w->n1, (const Words8 *)src[k], w->n, dst[k], w->n, e.view.d_flag);
  }
  if (phase != 2) wit_phase(e, w, nb, 1, run, nullptr);
  if (phase != 1) wit_phase(e, w, nb, 2, run, chi ? run.chi : nullptr);
  const size_t lo = phase == 2 ? w->n1 : 0, hi = phase == 1 ? w->n1 : w->n;
  wit_export(e, w, nb, run, lo, hi - lo, (Words8 *)aL + lo, (Words8 *)aR + lo, (Words8 *)aO + lo, w->n);
  return bpgpu_internal_hip(e.ctx, hipGetLastError(), "witness synthesis launch");
}

// ---- bpgpu_r1cs_prove_fs2 ----
struct Fs2Io {
  const void *states_in;
  const uint8_t *gadget_label;
  const void *v, *inputs, *s_L, *s_R, *vector_keys, *v_blinding, *blindings;
  void *proof_points, *proof_scalars, *wire, *challenges_out, *states_out, *chi_out, *aL, *aR, *aO;
};
size_t lg_padded(size_t n) {
  size_t k = 0;
  while (((size_t)1 << k) < n) k++;
  return k;
}
// what bpgpu_r1cs_prove_fs2 and bpgpu_r1cs_prove_values share: is w the program of c?
bool wit_program_of(const bpgpu_witness *w, const bpgpu_circuit *c) {
  size_t n, m, nchi;
  bpgpu_internal_circuit_dims(c, &n, &m, &nchi);
  return w->n == n && w->m == m && w->nchi == nchi;
}
// ... and what a prover on a gate program requires of its pointers, whatever the circuit's shape (nb > 0; the label is the caller's)
int wit_prover_pointers(const bpgpu_witness *w, size_t nb, const Fs2Io &a) {
  if (!a.states_in || !a.blindings || !a.proof_points || !a.proof_scalars || (w->m && (!a.v || !a.v_blinding)) || (w->ninp && !a.inputs))
    return BPGPU_E_ARG;
  if ((!a.s_L) != (!a.s_R) || (a.s_L != nullptr) == (a.vector_keys != nullptr)) return BPGPU_E_ARG;   // exactly one source of s_L, s_R
  if ((!a.aL) != (!a.aR) || (!a.aL) != (!a.aO)) return BPGPU_E_ARG;                                    // the three planes, or none
  return wit_fits(w, nb) ? BPGPU_OK : BPGPU_E_LEN;
}
int fs2_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb, const Fs2Io &a) {
  if (!ctx || !g || !c || !w) return BPGPU_E_ARG;
  if (!wit_program_of(w, c)) return BPGPU_E_ARG;
  WCK(bpgpu_internal_prove_fs2_labels(c, a.gadget_label, false));
  WCK(bpgpu_internal_prove_fs2_shape(g, c, nb, w->n1));
  if (!nb) return BPGPU_OK;
  WCK(bpgpu_internal_prove_fs2_labels(c, a.gadget_label, true));   // the call's label, unless the circuit has its own
  return wit_prover_pointers(w, nb, a);
}
struct Fs2Between { const Entered *e; const bpgpu_witness *w; size_t nb; const WitRun *run; void *L2, *R2, *O2; };
int fs2_between(void *user, const void *chi_dev) {
  const Fs2Between &b = *(const Fs2Between *)user;
  const size_t n2 = b.w->n - b.w->n1;
  wit_phase(*b.e, b.w, b.nb, 2, *b.run, (const Words8 *)chi_dev);
  wit_export(*b.e, b.w, b.nb, *b.run, b.w->n1, n2, b.L2, b.R2, b.O2, n2);
  return BPGPU_OK;
}
// mutex held, arguments checked, nb > 0; every pointer but the label HBM; asynchronous
int fs2_locked(const Entered &e, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb, const Fs2Io &io) {
  if (e.view.shard_world > 1) return BPGPU_E_ARG;      // partial sums cannot be hashed
  const size_t n = w->n, n1 = w->n1, n2 = n - n1;
  hipStream_t st = e.view.st;
  Scratch sc(e.ctx);
  WitRun run;
  WCK(wit_begin(e, w, nb, io.v, io.inputs, sc, &run));
  // the operands as the two chains take them, a phase each: witness planes and blinding vectors nb x n1 | nb x n2, keys nb x 32 each,
  // blinding factors nb x 3 | nb x 8
  const bool vec = io.s_L != nullptr;
  const size_t p1 = nb * n1, p2 = nb * n2;
  Words8 *split = (Words8 *)sc.take(((vec ? 5 : 3) * (p1 + p2) + 2 * nb + 11 * nb) * 32);
  if (!split) return BPGPU_E_OOM;
  Words8 *at = split;
  auto cut = [&](size_t count) { Words8 *p = at; at += count; return p; };
  Words8 *L1 = cut(p1), *R1 = cut(p1), *O1 = cut(p1), *L2 = cut(p2), *R2 = cut(p2), *O2 = cut(p2);
  Words8 *sL1 = vec ? cut(p1) : nullptr, *sR1 = vec ? cut(p1) : nullptr, *sL2 = vec ? cut(p2) : nullptr, *sR2 = vec ? cut(p2) : nullptr;
  Words8 *k1 = cut(nb), *k2 = cut(nb), *bl1 = cut(3 * nb), *bl2 = cut(8 * nb);
  auto rows = [&](void *dst, size_t dcount, const void *src, size_t scount, size_t off) {   // dcount scalars of each prover's scount, from off
    if (!dcount) return hipSuccess;
    return hipMemcpy2DAsync(dst, dcount * 32, (const Words8 *)src + off, scount * 32, dcount * 32, nb, hipMemcpyDeviceToDevice, st);
  };
  if (vec) {
    WHIP(e.ctx, rows(sL1, n1, io.s_L, n, 0));
    WHIP(e.ctx, rows(sR1, n1, io.s_R, n, 0));
    WHIP(e.ctx, rows(sL2, n2, io.s_L, n, n1));
    WHIP(e.ctx, rows(sR2, n2, io.s_R, n, n1));
  } else {
    WHIP(e.ctx, rows(k1, 1, io.vector_keys, 2, 0));
    WHIP(e.ctx, rows(k2, 1, io.vector_keys, 2, 1));
  }
  WHIP(e.ctx, rows(bl1, 3, io.blindings, 11, 0));
  WHIP(e.ctx, rows(bl2, 8, io.blindings, 11, 3));
  wit_phase(e, w, nb, 1, run, nullptr);
  wit_export(e, w, nb, run, 0, n1, L1, R1, O1, n1);
  const Fs2Between b{&e, w, nb, &run, L2, R2, O2};
  const bpgpu_internal_fs2 ch{io.states_in, io.gadget_label,
                              n1 ? L1 : nullptr, n1 ? R1 : nullptr, n1 ? O1 : nullptr, sL1, sR1, vec ? nullptr : k1, bl1,
                              L2, R2, O2, sL2, sR2, vec ? nullptr : k2, bl2,
                              io.v_blinding, io.proof_points, io.proof_scalars, io.wire, io.challenges_out, io.states_out, io.chi_out};
  WCK(bpgpu_internal_prove_fs2_chains(e.ctx, g, c, nb, n1, ch, fs2_between, (void *)&b));
  if (io.aL) wit_export(e, w, nb, run, 0, n, io.aL, io.aR, io.aO, n);
  return bpgpu_internal_hip(e.ctx, hipGetLastError(), "two-phase prover launch");
}

// ---- bpgpu_r1cs_prove_values ----
using PvIo = bpgpu_internal_pv;
int pv_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb, const PvIo &a) {
  if (!ctx || !g || !c || !w) return BPGPU_E_ARG;
  if (!wit_program_of(w, c)) return BPGPU_E_ARG;                                      // not this circuit's program
  const bool two = w->nchi != 0;
  if (!two && w->n1 != w->n) return BPGPU_E_ARG;
  if (two) WCK(bpgpu_internal_prove_fs2_labels(c, a.gadget_label, false));            // several challenges: only with the circuit's own labels
  WCK(two ? bpgpu_internal_prove_fs2_shape(g, c, nb, w->n1) : bpgpu_internal_prove_fs_shape(g, c, nb));
  WCK(bpgpu_internal_commit_values_shape(nb, w->m));
  if (!nb) return BPGPU_OK;
  // the label goes with the gadget challenge: the call's, unless the circuit has its own
  if (two ? bpgpu_internal_prove_fs2_labels(c, a.gadget_label, true) != BPGPU_OK : a.gadget_label != nullptr) return BPGPU_E_ARG;
  if (bpgpu_internal_shard_world(ctx) > 1) return BPGPU_E_ARG;                        // partial sums cannot be hashed
  if (!a.ok) return BPGPU_E_ARG;
  return wit_prover_pointers(w, nb, {a.init_states, a.gadget_label, a.v, a.inputs, a.s_L, a.s_R, a.vector_keys, a.v_blinding, a.blindings,
                                     a.proof_points, a.proof_scalars, a.wire, a.challenges_out, a.states_out, a.gadget_challenges_out,
                                     a.a_L_out, a.a_R_out, a.a_O_out});
}
// what both forms do between taking the mutex and touching an operand: the shard refusal, and the one-time build of the circuit's
// row-major view (the one wait of the call) with the check's BPGPU_E_LEN -- before a copy or a launch is enqueued
int pv_enter(const Entered &e, const bpgpu_circuit *c, size_t nb) {
  if (e.view.shard_world > 1) return BPGPU_E_ARG;
  return bpgpu_internal_rows_fit(e.ctx, c, nb);
}
// Mutex held, arguments checked, the circuit's row-major view built (pv_enter), nb > 0; every pointer but the label HBM;
// asynchronous.  The stages are the _locked functions of the calls they replace; between them the chain states
// after the commitments, the witness planes and the gadget challenge stay in pool memory (or in the caller's buffers, where given).
int pv_locked(const Entered &e, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb, const PvIo &io) {
  bpgpu_ctx *ctx = e.ctx;
  const bool two = w->nchi != 0;
  const size_t n = w->n, m = w->m, k = lg_padded(n), plane = nb * n, nchis = nb * w->nchi;
  Scratch sc(ctx);
  Words8 *mid = (Words8 *)sc.take((nb + (two && !io.gadget_challenges_out ? nchis : 0) + (io.a_L_out ? 0 : 3 * plane)) * 32);
  if (!mid) return BPGPU_E_OOM;
  Words8 *at = mid + nb;
  void *chi = nullptr, *L = io.a_L_out, *R = io.a_R_out, *O = io.a_O_out;
  if (two) { chi = io.gadget_challenges_out; if (!chi) { chi = at; at += nchis; } }
  if (!L) { L = at; R = at + plane; O = at + 2 * plane; }
  WCK(bpgpu_internal_commit_values(ctx, g, nb, m, io.v, io.v_blinding, io.init_states, io.V, io.V_compressed, mid));
  if (!two) {
    WCK(synth_locked(e, w, nb, 0, io.v, io.inputs, nullptr, L, R, O));
    WCK(bpgpu_internal_constraints_satisfied(ctx, c, nb, L, R, O, io.v, nullptr, io.ok, io.first_bad_row, io.first_bad_gate));
    WCK(bpgpu_internal_prove_fs(ctx, g, c, nb, {mid, L, R, O, io.s_L, io.s_R, io.vector_keys, io.v_blinding, io.blindings, io.proof_points,
                                                io.proof_scalars, io.wire, io.challenges_out, io.states_out}));
  } else {
    // (the phase-2 witness does not exist before the gadget challenge: the check follows the proof)
    WCK(fs2_locked(e, g, c, w, nb, {mid, io.gadget_label, io.v, io.inputs, io.s_L, io.s_R, io.vector_keys, io.v_blinding, io.blindings,
                                    io.proof_points, io.proof_scalars, io.wire, io.challenges_out, io.states_out, chi, L, R, O}));
    WCK(bpgpu_internal_constraints_satisfied(ctx, c, nb, L, R, O, io.v, chi, io.ok, io.first_bad_row, io.first_bad_gate));
  }
  {
    Prof22 prof(ctx);
    prove_fs_clear_rejected(e.view.st, {nb, (11 + 2 * k) * 64, (5 + k) * 32, 1 + (two ? 14 : 11) * 32 + (2 * k + 2) * 32, (const int32_t *)io.ok,
                                        (uint8_t *)io.proof_points, (uint8_t *)io.proof_scalars, (uint8_t *)io.challenges_out,
                                        (uint8_t *)io.states_out, (uint8_t *)io.wire});
  }
  return bpgpu_internal_hip(ctx, hipGetLastError(), "prove-from-values launch");
}

}  // namespace

size_t bpgpu_internal_witness_inputs(const bpgpu_witness *w) { return w->ninp; }
int bpgpu_internal_prove_values_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                                      const bpgpu_internal_pv &a) {
  return pv_check(ctx, g, c, w, nb, a);
}

int bpgpu_internal_witness_levels(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                                  const uint32_t *idx, uint32_t *level) {
  WitShape s;
  WCK(wit_analyse(n, n1, nchi, op, row_ptr, kind, idx, &s));
  std::copy(s.level.begin(), s.level.end(), level);
  return BPGPU_OK;
}

extern "C" {
#pragma GCC visibility push(default)

int bpgpu_witness_plan(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                       size_t nb, int32_t out[BPGPU_WIT_PLAN_FIELDS]) {
  return no_throw([&]() -> int {
    if (!out) return BPGPU_E_ARG;
    WitShape s;
    WCK(wit_analyse(n, n1, nchi, op, row_ptr, kind, idx, &s));
    out[BPGPU_WIT_PLAN_LEVELS1] = (int32_t)s.levels[0];
    out[BPGPU_WIT_PLAN_LEVELS2] = (int32_t)s.levels[1];
    out[BPGPU_WIT_PLAN_WIDEST] = (int32_t)s.widest;
    out[BPGPU_WIT_PLAN_LONG_ROWS] = (int32_t)s.nlong;
    out[BPGPU_WIT_PLAN_INPUTS] = (int32_t)s.ninp;
    out[BPGPU_WIT_PLAN_ROUTE1] = wit_route_scan(n1, s.levels[0], s.longest[0], s.xlongest[0], nb, WIT_SCAN_MIN_DEFAULT);
    out[BPGPU_WIT_PLAN_ROUTE2] = wit_route_scan(n - n1, s.levels[1], s.longest[1], s.xlongest[1], nb, WIT_SCAN_MIN_DEFAULT);
    return BPGPU_OK;
  });
}
int bpgpu_witness_affine_chains(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                                const uint32_t *idx, int32_t out[BPGPU_WIT_AFF_FIELDS]) {
  return no_throw([&]() -> int {
    if (!out) return BPGPU_E_ARG;
    WitShape s;
    WCK(wit_analyse(n, n1, nchi, op, row_ptr, kind, idx, &s));
    for (int ph = 0; ph < 2; ph++) {
      out[BPGPU_WIT_AFF_CHAINS1 + ph] = (int32_t)s.xchains[ph];
      out[BPGPU_WIT_AFF_MEMBERS1 + ph] = (int32_t)s.xmembers[ph];
      out[BPGPU_WIT_AFF_AFFINE1 + ph] = (int32_t)s.xaffine[ph];
      out[BPGPU_WIT_AFF_LONGEST1 + ph] = (int32_t)s.xlongest[ph];
      out[BPGPU_WIT_AFF_LEVELS1 + ph] = (int32_t)s.xscan_levels[ph];
    }
    return BPGPU_OK;
  });
}
int bpgpu_witness_chains(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                         const uint32_t *idx, int32_t out[BPGPU_WIT_CHAIN_FIELDS]) {
  return no_throw([&]() -> int {
    if (!out) return BPGPU_E_ARG;
    WitShape s;
    WCK(wit_analyse(n, n1, nchi, op, row_ptr, kind, idx, &s));
    for (int ph = 0; ph < 2; ph++) {
      out[BPGPU_WIT_CHAIN_CHAINS1 + ph] = (int32_t)s.chains[ph];
      out[BPGPU_WIT_CHAIN_MEMBERS1 + ph] = (int32_t)s.members[ph];
      out[BPGPU_WIT_CHAIN_LONGEST1 + ph] = (int32_t)s.longest[ph];
      out[BPGPU_WIT_CHAIN_LEVELS1 + ph] = (int32_t)s.scan_levels[ph];
    }
    return BPGPU_OK;
  });
}

int bpgpu_witness_create(bpgpu_ctx *ctx, size_t n, size_t n1, size_t m, size_t nchi, const uint8_t *op, const uint32_t *arg,
                         const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx, const uint8_t *coeff, bpgpu_witness **out) {
  return no_throw([&]() -> int {
    if (!ctx || !out) return BPGPU_E_ARG;
    *out = nullptr;
    if (n && !arg) return BPGPU_E_ARG;
    WitShape s;
    WCK(wit_analyse(n, n1, nchi, op, row_ptr, kind, idx, &s));
    if (m > ROWS_IDX_MASK) return BPGPU_E_LEN;
    if (s.nnz && !coeff) return BPGPU_E_ARG;
    const size_t rows = 2 * n, nnz = s.nnz, nlev = (size_t)s.levels[0] + s.levels[1];
    // the rest of the validation: after it no index a kernel forms is out of range
    for (size_t i = 0; i < n; i++) {
      if (op[i] == BPGPU_GATE_BIT && arg[i] >= WIT_BIT_MAX) return BPGPU_E_ARG;
      if (op[i] == BPGPU_GATE_INPUT && (s.row_len[2 * i] || s.row_len[2 * i + 1])) return BPGPU_E_ARG;
      if ((op[i] == BPGPU_GATE_BIT || op[i] == BPGPU_GATE_INV) && s.row_len[2 * i + 1]) return BPGPU_E_ARG;
      for (size_t j = 0; j <= nchi; j++) {
        const size_t r = j * rows + 2 * i;
        if (j && i < n1 && row_ptr[r + 2] != row_ptr[r]) return BPGPU_E_ARG;       // the challenge does not exist in phase 1
        for (uint32_t t = row_ptr[r]; t < row_ptr[r + 2]; t++)
          if (kind[t] == 3 && idx[t] >= m) return BPGPU_E_ARG;
      }
    }
    // the image of the device arrays: [coeff | row_ptr | var | arg | order | level_ptr | level_long | op | scan_order | scan_ptr |
    // scan_long | chain_elem | chain_ptr | slot | asc | level_inv | scan_inv], every part 256-byte aligned
    const size_t nslev = (size_t)s.xscan_levels[0] + s.xscan_levels[1];
    const size_t o_rp = up256((nnz ? nnz : 1) * 32), o_var = o_rp + up256((rows + 1) * 4), o_arg = o_var + up256((nnz ? nnz : 1) * 4),
                 o_ord = o_arg + up256((n ? n : 1) * 4), o_lp = o_ord + up256((n ? n : 1) * 4), o_ll = o_lp + up256((nlev + 1) * 4),
                 o_op = o_ll + up256((nlev ? nlev : 1) * 4), o_so = o_op + up256(n ? n : 1), o_sp = o_so + up256((n ? n : 1) * 4),
                 o_sl = o_sp + up256((nslev + 1) * 4), o_ce = o_sl + up256((nslev ? nslev : 1) * 4), o_cp = o_ce + up256((n ? n : 1) * 4),
                 o_slot = o_cp + up256((nslev + 1) * 4), o_asc = o_slot + up256((n ? n : 1) * 4), o_li = o_asc + up256((n ? n : 1) * 4),
                 o_si = o_li + up256((nlev ? nlev : 1) * 4), total = o_si + up256((nslev ? nslev : 1) * 4);
    std::vector<uint8_t> img(total, 0);
    Words8 *h_coeff = (Words8 *)img.data();
    uint32_t *h_rp = (uint32_t *)(img.data() + o_rp), *h_var = (uint32_t *)(img.data() + o_var), *h_arg = (uint32_t *)(img.data() + o_arg),
             *h_ord = (uint32_t *)(img.data() + o_ord), *h_lp = (uint32_t *)(img.data() + o_lp), *h_ll = (uint32_t *)(img.data() + o_ll);
    uint8_t *h_op = img.data() + o_op;
    // one CSR of 2 n rows: a row's blocks one after the other, the block in the term's code; coefficients in Montgomery form
    uint32_t pos = 0;
    for (size_t r = 0; r < rows; r++) {
      h_rp[r] = pos;
      for (size_t j = 0; j <= nchi; j++)
        for (uint32_t t = row_ptr[j * rows + r]; t < row_ptr[j * rows + r + 1]; t++, pos++) {
          uint32_t cw[8];
          memcpy(cw, coeff + 32 * (size_t)t, 32);
          if (!words_lt_mod<FN>(cw)) return BPGPU_E_ARG;
          pack(h_coeff[pos].w, canon(to_mont(unpack<FN>(cw))));
          h_var[pos] = (kind[t] == 4 ? 0u : idx[t]) | kind[t] << ROWS_KIND_SHIFT | (uint32_t)j << ROWS_CHI_SHIFT;
        }
    }
    h_rp[rows] = pos;
    // an affine member's link term first in its link row (wit_link reads a row's first term; the sums are exact: the order is free)
    for (size_t i = 0; i < n; i++) {
      if (!s.is_affine[i]) continue;
      const uint32_t lo = h_rp[2 * i + s.xlink_right[i]], hi = h_rp[2 * i + s.xlink_right[i] + 1], phase_lo = i < n1 ? 0 : (uint32_t)n1;
      for (uint32_t t = lo; t < hi; t++)
        if (((h_var[t] >> ROWS_KIND_SHIFT) & 7u) <= 2 && (h_var[t] & ROWS_IDX_MASK) >= phase_lo) {
          std::swap(h_var[t], h_var[lo]);
          std::swap(h_coeff[t], h_coeff[lo]);
          break;
        }
    }
    // the gates of a phase sorted by level (stable: program order within a level): the ones with short rows, the INV gates among
    // them last (k_witness.hip inverts once per thread for those), then the ones with a long row.  A level without an INV gate has
    // the order it always had
    const uint32_t lane_max = rows_lane_max();
    uint32_t *h_li = (uint32_t *)(img.data() + o_li), *h_si = (uint32_t *)(img.data() + o_si);
    const auto list_of = [&](size_t i) {        // 0: short rows | 1: short rows, INV | 2: a long row
      if (s.row_len[2 * i] > lane_max || s.row_len[2 * i + 1] > lane_max) return 2;
      return op[i] == BPGPU_GATE_INV ? 1 : 0;
    };
    uint32_t pairs = 0, at = 0, lvl_base = 0;
    for (size_t i = 0; i < n; i++) {
      h_op[i] = op[i];
      h_arg[i] = op[i] == BPGPU_GATE_INPUT ? pairs++ : (op[i] == BPGPU_GATE_BIT ? arg[i] : 0);
    }
    for (int ph = 0; ph < 2; ph++) {
      const size_t lo = ph ? n1 : 0, hi = ph ? n : n1;
      for (uint32_t l = 0; l < s.levels[ph]; l++) {
        h_lp[lvl_base + l] = at;
        for (int list = 0; list < 3; list++) {
          if (list == 1) h_li[lvl_base + l] = at;
          if (list == 2) h_ll[lvl_base + l] = at;
          for (size_t i = lo; i < hi; i++)
            if (s.level[i] == l && list_of(i) == list) h_ord[at++] = (uint32_t)i;
        }
      }
      lvl_base += s.levels[ph];
    }
    h_lp[nlev] = at;
    // a level's gates numbered by ascending gate index (the slots of the two-party form): each of its three runs in order[]
    // ascends, so the numbering is their merge
    uint32_t *h_slot = (uint32_t *)(img.data() + o_slot), *h_asc = (uint32_t *)(img.data() + o_asc);
    for (size_t l = 0; l < nlev; l++) {
      uint32_t at3[3] = {h_lp[l], h_li[l], h_ll[l]};
      const uint32_t end3[3] = {h_li[l], h_ll[l], h_lp[l + 1]};
      for (uint32_t t = h_lp[l]; t < h_lp[l + 1]; t++) {
        int from = -1;
        for (int k = 0; k < 3; k++)
          if (at3[k] < end3[k] && (from < 0 || h_ord[at3[k]] < h_ord[at3[from]])) from = k;
        const uint32_t u = at3[from]++;
        h_slot[u] = t - h_lp[l];
        h_asc[t] = h_ord[u];
      }
    }
    // the same over the extended compressed levels, members apart: a level's ordinary gates (short rows, INV last; then long), and the members
    // of the extended chains it heads, chain after chain (heads in program order), each chain from its first member on.  A phase
    // without an affine member has the product chains' lists: pass 2 changed nothing of it
    uint32_t *h_so = (uint32_t *)(img.data() + o_so), *h_sp = (uint32_t *)(img.data() + o_sp), *h_sl = (uint32_t *)(img.data() + o_sl),
             *h_ce = (uint32_t *)(img.data() + o_ce), *h_cp = (uint32_t *)(img.data() + o_cp);
    std::vector<uint32_t> fill(4 * nslev + 1, 0);          // per compressed level: short, INV, long, members -> where each list starts
    const auto slot = [&](size_t i) {
      const size_t l = (i < n1 ? 0 : s.xscan_levels[0]) + s.xscan_level[i];
      return 4 * l + (s.xpred[i] != WIT_NONE ? 3 : list_of(i));          // (an INV gate is never a member)
    };
    for (size_t i = 0; i < n; i++) fill[slot(i) + 1]++;
    uint32_t ord_at = 0, mem_at = 0;
    for (size_t l = 0; l < nslev; l++) {
      const uint32_t shorts = fill[4 * l + 1], invs = fill[4 * l + 2], longs = fill[4 * l + 3], mems = fill[4 * l + 4];
      h_sp[l] = ord_at; h_si[l] = ord_at + shorts; h_sl[l] = ord_at + shorts + invs; h_cp[l] = mem_at;
      fill[4 * l] = ord_at; fill[4 * l + 1] = ord_at + shorts; fill[4 * l + 2] = ord_at + shorts + invs; fill[4 * l + 3] = mem_at;
      ord_at += shorts + invs + longs;
      mem_at += mems;
    }
    h_sp[nslev] = ord_at; h_cp[nslev] = mem_at;
    for (size_t i = 0; i < n; i++) {
      if (s.xpred[i] != WIT_NONE) continue;
      const size_t k = slot(i);
      h_so[fill[k]++] = (uint32_t)i;
      if (s.xsucc[i] == WIT_NONE) continue;
      uint32_t &m_at = fill[k - k % 4 + 3];                 // a head: its chain, whole, into its level's member list
      for (uint32_t e = s.xsucc[i], first = WIT_ELEM_START; e != WIT_NONE; e = s.xsucc[e], first = 0)
        h_ce[m_at++] = e | first | (s.xlink_right[e] ? WIT_ELEM_RIGHT : 0u) | (s.is_affine[e] ? WIT_ELEM_AFFINE : 0u);
    }
    bpgpu_witness *w = new (std::nothrow) bpgpu_witness();
    if (!w) return BPGPU_E_OOM;
    w->n = n; w->n1 = n1; w->m = m; w->nchi = nchi; w->ninp = s.ninp;
    w->levels[0] = s.levels[0]; w->levels[1] = s.levels[1];
    for (size_t i = 0; i < n; i++) if (op[i] == BPGPU_GATE_BIT) w->bits[i < n1 ? 0 : 1]++;
    w->invs[0] = s.ninv[0]; w->invs[1] = s.ninv[1];
    w->divs[0] = s.ndiv[0]; w->divs[1] = s.ndiv[1];
    w->level_ptr.assign(h_lp, h_lp + nlev + 1);
    w->level_long.assign(h_ll, h_ll + nlev);
    for (int ph = 0; ph < 2; ph++) {
      w->scan_levels[ph] = s.xscan_levels[ph]; w->longest[ph] = s.longest[ph];
      w->xlongest[ph] = s.xlongest[ph]; w->affine[ph] = s.xaffine[ph] != 0;
    }
    Entered e(ctx);
    int rc = e.enter();
    // (a plain allocation, not the context's pool: a program may outlive the context that made it, as a circuit may)
    if (rc == BPGPU_OK && hipMalloc(&w->mem, total) != hipSuccess) { (void)hipGetLastError(); w->mem = nullptr; rc = BPGPU_E_OOM; }
    if (rc == BPGPU_OK) rc = bpgpu_internal_hip(ctx, hipMemcpyAsync(w->mem, img.data(), total, hipMemcpyHostToDevice, e.view.st), "witness program upload");
    if (rc == BPGPU_OK) rc = bpgpu_internal_hip(ctx, hipStreamSynchronize(e.view.st), "witness program upload");     // `img` is a local
    if (rc != BPGPU_OK) { if (w->mem) (void)hipFree(w->mem); delete w; return rc; }
    const uint8_t *d = (const uint8_t *)w->mem;
    w->dev.rows = RowsDev{(const uint32_t *)(d + o_rp), (const uint32_t *)(d + o_var), (const Words8 *)d, nullptr, rows, nnz, 0};
    w->dev.op = d + o_op;
    w->dev.arg = (const uint32_t *)(d + o_arg);
    w->dev.order = (const uint32_t *)(d + o_ord);
    w->dev.level_ptr = (const uint32_t *)(d + o_lp);
    w->dev.level_long = (const uint32_t *)(d + o_ll);
    w->dev.scan_order = (const uint32_t *)(d + o_so);
    w->dev.scan_ptr = (const uint32_t *)(d + o_sp);
    w->dev.scan_long = (const uint32_t *)(d + o_sl);
    w->dev.chain_elem = (const uint32_t *)(d + o_ce);
    w->dev.chain_ptr = (const uint32_t *)(d + o_cp);
    w->dev.slot = (const uint32_t *)(d + o_slot);
    w->dev.asc = (const uint32_t *)(d + o_asc);
    w->dev.level_inv = (const uint32_t *)(d + o_li);
    w->dev.scan_inv = (const uint32_t *)(d + o_si);
    w->dev.n = (uint32_t)n; w->dev.m = (uint32_t)m; w->dev.nchi = (uint32_t)nchi; w->dev.ninp = s.ninp;
    *out = w;
    return BPGPU_OK;
  });
}
void bpgpu_witness_destroy(bpgpu_ctx *ctx, bpgpu_witness *w) {
  if (!w) return;
  if (ctx) (void)bpgpu_sync(ctx);
  (void)hipFree(w->mem);
  delete w;
}

int bpgpu_r1cs_witness_synthesize_dev(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const void *v, const void *inputs,
                                      const void *gadget_challenges, void *a_L, void *a_R, void *a_O) {
  return no_throw([&]() -> int {
    WCK(synth_check(ctx, w, nb, phase, v, inputs, gadget_challenges, a_L, a_R, a_O));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    WCK(bpgpu_internal_flag_reset(ctx));   // the flag reports on the most recent *_dev call
    return synth_locked(e, w, nb, phase, v, inputs, gadget_challenges, a_L, a_R, a_O);
  });
}
int bpgpu_r1cs_witness_synthesize(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const uint8_t *v, const uint8_t *inputs,
                                  const uint8_t *gadget_challenges, uint8_t *a_L, uint8_t *a_R, uint8_t *a_O) {
  return no_throw([&]() -> int {
    WCK(synth_check(ctx, w, nb, phase, v, inputs, gadget_challenges, a_L, a_R, a_O));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    Scratch sc(ctx);
    // staging: the three planes, then v, the input pairs, the challenges
    const size_t plane = nb * w->n, b_v = nb * w->m * 32, b_in = 2 * nb * w->ninp * 32, b_chi = gadget_challenges ? nb * w->nchi * 32 : 0;
    Words8 *dL = (Words8 *)sc.take(3 * plane * 32 + b_v + b_in + b_chi);
    if (!dL) return BPGPU_E_OOM;
    Words8 *dR = dL + plane, *dO = dR + plane;
    uint8_t *dv = (uint8_t *)(dO + plane), *din = dv + b_v, *dchi = din + b_in;
    hipStream_t st = e.view.st;
    WCK(bpgpu_internal_flag_reset(ctx));
    if (b_v) WHIP(ctx, hipMemcpyAsync(dv, v, b_v, hipMemcpyHostToDevice, st));
    if (b_in) WHIP(ctx, hipMemcpyAsync(din, inputs, b_in, hipMemcpyHostToDevice, st));
    if (b_chi) WHIP(ctx, hipMemcpyAsync(dchi, gadget_challenges, b_chi, hipMemcpyHostToDevice, st));
    uint8_t *host[3] = {a_L, a_R, a_O};
    Words8 *dev[3] = {dL, dR, dO};
    // a phase on its own leaves the other phase's multipliers as the caller holds them: the planes travel whole, both ways
    if (phase != 0 && plane) for (int k = 0; k < 3; k++) WHIP(ctx, hipMemcpyAsync(dev[k], host[k], plane * 32, hipMemcpyHostToDevice, st));
    WCK(synth_locked(e, w, nb, phase, b_v ? dv : nullptr, b_in ? din : nullptr, b_chi ? dchi : nullptr, dL, dR, dO));
    WCK(bpgpu_internal_checked_wait(ctx));
    if (plane) for (int k = 0; k < 3; k++) WHIP(ctx, hipMemcpyAsync(host[k], dev[k], plane * 32, hipMemcpyDeviceToHost, st));
    WHIP(ctx, hipStreamSynchronize(st));
    return BPGPU_OK;
  });
}

int bpgpu_r1cs_prove_fs2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                             const void *states_in, const uint8_t gadget_label[32], const void *v, const void *inputs, const void *s_L,
                             const void *s_R, const void *vector_keys, const void *v_blinding, const void *blindings, void *proof_points,
                             void *proof_scalars, void *wire, void *challenges_out, void *states_out, void *gadget_challenges_out,
                             void *a_L_out, void *a_R_out, void *a_O_out) {
  return no_throw([&]() -> int {
    const Fs2Io io{states_in, gadget_label, v, inputs, s_L, s_R, vector_keys, v_blinding, blindings, proof_points, proof_scalars, wire,
                   challenges_out, states_out, gadget_challenges_out, a_L_out, a_R_out, a_O_out};
    WCK(fs2_check(ctx, g, c, w, nb, io));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    WCK(bpgpu_internal_flag_reset(ctx));   // the flag reports on the most recent *_dev call
    return fs2_locked(e, g, c, w, nb, io);
  });
}
int bpgpu_r1cs_prove_fs2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                         const uint8_t *states_in, const uint8_t gadget_label[32], const uint8_t *v, const uint8_t *inputs, const uint8_t *s_L,
                         const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *v_blinding, const uint8_t *blindings,
                         uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out,
                         uint8_t *gadget_challenges_out, uint8_t *a_L_out, uint8_t *a_R_out, uint8_t *a_O_out) {
  return no_throw([&]() -> int {
    const Fs2Io a{states_in, gadget_label, v, inputs, s_L, s_R, vector_keys, v_blinding, blindings, proof_points, proof_scalars, wire,
                  challenges_out, states_out, gadget_challenges_out, a_L_out, a_R_out, a_O_out};
    WCK(fs2_check(ctx, g, c, w, nb, a));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    if (e.view.shard_world > 1) return BPGPU_E_ARG;
    Scratch sc(ctx);
    const size_t n = w->n, m = w->m, k = lg_padded(n), plane = nb * n * 32;
    // staging: the operands in the order given (an absent one, of zero bytes, gets a null device pointer), then the results -- the
    // optional ones downloaded only when asked for, the wire form (of odd length) last
    const void *in_host[8] = {a.states_in, a.v, a.inputs, a.s_L, a.s_R, a.vector_keys, a.v_blinding, a.blindings};
    const size_t in_bytes[8] = {nb * 32, nb * m * 32, 2 * nb * w->ninp * 32, a.s_L ? plane : 0, a.s_R ? plane : 0, a.vector_keys ? nb * 64 : 0,
                                nb * m * 32, nb * 11 * 32};
    void *out_host[9] = {a.proof_points, a.proof_scalars, a.challenges_out, a.states_out, a.chi_out, a.aL, a.aR, a.aO, a.wire};
    const size_t out_bytes[9] = {nb * (11 + 2 * k) * 64, nb * 5 * 32, a.challenges_out ? nb * (5 + k) * 32 : 0, a.states_out ? nb * 32 : 0,
                                 a.chi_out ? nb * w->nchi * 32 : 0, a.aL ? plane : 0, a.aL ? plane : 0, a.aL ? plane : 0,
                                 a.wire ? nb * (1 + 14 * 32 + (2 * k + 2) * 32) : 0};
    size_t total = 0;
    for (size_t b : in_bytes) total += b;
    for (size_t b : out_bytes) total += b;
    uint8_t *stage = (uint8_t *)sc.take(total);
    if (!stage) return BPGPU_E_OOM;
    uint8_t *in[8], *out[9], *at = stage;
    for (int i = 0; i < 8; i++) { in[i] = in_bytes[i] ? at : nullptr; at += in_bytes[i]; }
    for (int i = 0; i < 9; i++) { out[i] = out_bytes[i] ? at : nullptr; at += out_bytes[i]; }
    hipStream_t st = e.view.st;
    WCK(bpgpu_internal_flag_reset(ctx));
    for (int i = 0; i < 8; i++) if (in_bytes[i]) WHIP(ctx, hipMemcpyAsync(in[i], in_host[i], in_bytes[i], hipMemcpyHostToDevice, st));
    WCK(fs2_locked(e, g, c, w, nb, {in[0], a.gadget_label, in[1], in[2], in[3], in[4], in[5], in[6], in[7], out[0], out[1], out[8], out[2],
                                    out[3], out[4], out[5], out[6], out[7]}));
    WCK(bpgpu_internal_checked_wait(ctx));
    for (int i = 0; i < 9; i++) if (out_bytes[i]) WHIP(ctx, hipMemcpyAsync(out_host[i], out[i], out_bytes[i], hipMemcpyDeviceToHost, st));
    WHIP(ctx, hipStreamSynchronize(st));
    return BPGPU_OK;
  });
}

int bpgpu_r1cs_prove_values_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                                const void *init_states, const uint8_t gadget_label[32], const void *v, const void *v_blinding,
                                const void *inputs, const void *s_L, const void *s_R, const void *vector_keys, const void *blindings, void *V,
                                void *V_compressed, void *ok, void *first_bad_row, void *first_bad_gate, void *proof_points, void *proof_scalars,
                                void *wire, void *challenges_out, void *states_out, void *gadget_challenges_out, void *a_L_out, void *a_R_out,
                                void *a_O_out) {
  return no_throw([&]() -> int {
    const PvIo io{init_states, gadget_label, v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, V, V_compressed, ok, first_bad_row,
                  first_bad_gate, proof_points, proof_scalars, wire, challenges_out, states_out, gadget_challenges_out, a_L_out, a_R_out, a_O_out};
    WCK(pv_check(ctx, g, c, w, nb, io));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    WCK(pv_enter(e, c, nb));
    WCK(bpgpu_internal_flag_reset(ctx));   // the flag reports on the most recent *_dev call
    return pv_locked(e, g, c, w, nb, io);
  });
}
int bpgpu_r1cs_prove_values(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                            const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *v, const uint8_t *v_blinding,
                            const uint8_t *inputs, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *blindings,
                            uint8_t *V, uint8_t *V_compressed, int32_t *ok, int64_t *first_bad_row, int64_t *first_bad_gate,
                            uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out,
                            uint8_t *gadget_challenges_out, uint8_t *a_L_out, uint8_t *a_R_out, uint8_t *a_O_out) {
  return no_throw([&]() -> int {
    const PvIo a{init_states, gadget_label, v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, V, V_compressed, ok, first_bad_row,
                 first_bad_gate, proof_points, proof_scalars, wire, challenges_out, states_out, gadget_challenges_out, a_L_out, a_R_out, a_O_out};
    WCK(pv_check(ctx, g, c, w, nb, a));
    if (!nb) return BPGPU_OK;
    Entered e(ctx);
    WCK(e.enter());
    WCK(pv_enter(e, c, nb));
    Scratch sc(ctx);
    const bool two = w->nchi != 0;
    const size_t n = w->n, m = w->m, k = lg_padded(n), plane = nb * n * 32;
    // staging: the operands in the header's order (an absent one, of zero bytes, gets a null device pointer), then the results -- the
    // optional ones downloaded only when asked for, every part 256-byte aligned (the verdict words and the wire form are no
    // multiples of 32 bytes).  What the provers send is a few scalars each; the planes never cross the bus unless asked for.
    const void *in_host[8] = {a.init_states, a.v, a.v_blinding, a.inputs, a.s_L, a.s_R, a.vector_keys, a.blindings};
    const size_t in_bytes[8] = {nb * 32, nb * m * 32, nb * m * 32, 2 * nb * w->ninp * 32, a.s_L ? plane : 0, a.s_R ? plane : 0,
                                a.vector_keys ? nb * (two ? 64 : 32) : 0, nb * (two ? 11 : 8) * 32};
    void *out_host[14] = {a.V, a.V_compressed, a.ok, a.first_bad_row, a.first_bad_gate, a.proof_points, a.proof_scalars, a.wire, a.challenges_out,
                          a.states_out, two ? a.gadget_challenges_out : nullptr, a.a_L_out, a.a_R_out, a.a_O_out};
    const size_t out_all[14] = {nb * m * 64, nb * m * 32, nb * 4, nb * 8, nb * 8, nb * (11 + 2 * k) * 64, nb * 5 * 32,
                                nb * (1 + (two ? 14 : 11) * 32 + (2 * k + 2) * 32), nb * (5 + k) * 32, nb * 32, nb * w->nchi * 32, plane, plane, plane};
    size_t out_bytes[14], total = 0;
    for (size_t b : in_bytes) total += up256(b);
    for (int i = 0; i < 14; i++) { out_bytes[i] = out_host[i] ? out_all[i] : 0; total += up256(out_bytes[i]); }
    uint8_t *stage = (uint8_t *)sc.take(total);
    if (!stage) return BPGPU_E_OOM;
    uint8_t *in[8], *out[14], *at = stage;
    for (int i = 0; i < 8; i++) { in[i] = in_bytes[i] ? at : nullptr; at += up256(in_bytes[i]); }
    for (int i = 0; i < 14; i++) { out[i] = out_bytes[i] ? at : nullptr; at += up256(out_bytes[i]); }
    hipStream_t st = e.view.st;
    WCK(bpgpu_internal_flag_reset(ctx));
    for (int i = 0; i < 8; i++) if (in_bytes[i]) WHIP(ctx, hipMemcpyAsync(in[i], in_host[i], in_bytes[i], hipMemcpyHostToDevice, st));
    const int rc = pv_locked(e, g, c, w, nb, {in[0], a.gadget_label, in[1], in[2], in[3], in[4], in[5], in[6], in[7], out[0], out[1], out[2], out[3],
                                              out[4], out[5], out[6], out[7], out[8], out[9], out[10], out[11], out[12], out[13]});
    if (rc != BPGPU_OK) {      // no copy from the caller's memory is left in flight behind an early return
      (void)hipStreamSynchronize(st);
      return rc;
    }
    WCK(bpgpu_internal_checked_wait(ctx));
    for (int i = 0; i < 14; i++) if (out_bytes[i]) WHIP(ctx, hipMemcpyAsync(out_host[i], out[i], out_bytes[i], hipMemcpyDeviceToHost, st));
    WHIP(ctx, hipStreamSynchronize(st));
    return BPGPU_OK;
  });
}

#pragma GCC visibility pop
}  // extern "C"
