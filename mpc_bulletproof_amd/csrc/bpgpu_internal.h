// bpgpu_internal.h -- what the translation units of libbpgpu.so share beside the public header: not exported.
#ifndef BPGPU_INTERNAL_H
#define BPGPU_INTERNAL_H
#include <hip/hip_runtime.h>
#include "../../include/bpgpu.h"

extern "C" {
// bpgpu_r1cs_verify_stream with the choice of its operand route handed in.  in_place_ok != 0: the public call's behaviour --
// page-locked operands are fetched in place over the bus (k_fetch3), pageable ones take the staged copies.  in_place_ok == 0: staged
// copies whatever the memory is.  bpgpu_pool.hip decides per slot: a device must not read host memory that is not mapped for it.
__attribute__((visibility("hidden"))) int bpgpu_internal_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                                                       size_t n1, size_t k, const uint8_t *points, const uint8_t *scalars,
                                                                       const uint8_t *challenges, int32_t *ok, int in_place_ok);
}

// ---- what bpgpu_witness.hip takes from bpgpu_api.hip, where bpgpu_ctx, its pool and the provers' chains live -------------------------
#define BPGPU_HIDDEN __attribute__((visibility("hidden")))
struct bpgpu_internal_view { hipStream_t st; int *d_flag; int64_t witness_route, witness_scan_min; size_t shard_world; };
// BPGPU_OPT_WITNESS_SCAN_MIN as a context starts with it, and as bpgpu_witness_plan (which has no context) reports routes
constexpr int64_t WIT_SCAN_MIN_DEFAULT = 16;
// from how many members of a phase's longest EXTENDED chain (product and affine members, bpgpu.h "affine member") the scan form is
// taken: max(BPGPU_OPT_WITNESS_SCAN_MIN, WIT_AFFINE_MIN).  Read from the sweep of profiles/witness_affine.log by the rule of the constant above
constexpr int64_t WIT_AFFINE_MIN = 16;
// an entry point's head and tail: the context's mutex taken and its device selected (on failure the mutex is free again) | released
BPGPU_HIDDEN int bpgpu_internal_enter(bpgpu_ctx *ctx, bpgpu_internal_view *view);
BPGPU_HIDDEN void bpgpu_internal_leave(bpgpu_ctx *ctx);
// the world of bpgpu_set_shard, for a refusal that must come before the device is selected
BPGPU_HIDDEN size_t bpgpu_internal_shard_world(bpgpu_ctx *ctx);
// between the two (mutex held): the context's buffer pool (nullptr: out of memory), the failure text of a HIP call -> BPGPU_E_*, a
// profile mark of `kind` on the stream (start and stop marks alternate), the input flag cleared, and the end of an entry point that
// waits: the launch check and the flag (BPGPU_E_ARG when raised), the stream drained
BPGPU_HIDDEN void *bpgpu_internal_pool_alloc(bpgpu_ctx *ctx, size_t bytes);
BPGPU_HIDDEN void bpgpu_internal_pool_release(bpgpu_ctx *ctx, void *p);
BPGPU_HIDDEN int bpgpu_internal_hip(bpgpu_ctx *ctx, hipError_t e, const char *what);
BPGPU_HIDDEN void bpgpu_internal_prof_mark(bpgpu_ctx *ctx, int kind);
BPGPU_HIDDEN int bpgpu_internal_flag_reset(bpgpu_ctx *ctx);
BPGPU_HIDDEN int bpgpu_internal_checked_wait(bpgpu_ctx *ctx);
// a circuit handle's shape, and the refusals of bpgpu_r1cs_prove_fs2_begin / _finish that depend on the shapes alone (BPGPU_OK with
// nb == 0: nothing to do)
BPGPU_HIDDEN void bpgpu_internal_circuit_dims(const bpgpu_circuit *c, size_t *n, size_t *m, size_t *nchi);
BPGPU_HIDDEN int bpgpu_internal_prove_fs2_shape(const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1);
// ... and on the circuit's labels: BPGPU_E_ARG for a numeric circuit, for a call's label beside attached ones
// (bpgpu_circuit_set_gadget_labels), and, with none attached, for nchi > 1 or (need_label) a null label
BPGPU_HIDDEN int bpgpu_internal_prove_fs2_labels(const bpgpu_circuit *c, const uint8_t *gadget_label, bool need_label);
// The chains of bpgpu_r1cs_prove_fs2_begin and _finish on one session that lives for the call (mutex held, shapes and arguments checked,
// nb > 0; every pointer but the label is HBM; asynchronous).  `between` runs once _begin's launches are enqueued, with the session's
// device copy of the gadget challenges (nb x nchi x 32, plain, prover-major): it enqueues whatever produces the phase-2 operands.
struct bpgpu_internal_fs2 {
  const void *states_in;
  const uint8_t *gadget_label;                                                  // host memory
  const void *a_L1, *a_R1, *a_O1, *s_L1, *s_R1, *keys1, *blindings1;            // nb x n1 | nb x 32 | nb x 3
  const void *a_L2, *a_R2, *a_O2, *s_L2, *s_R2, *keys2, *blindings2;            // nb x (n - n1) | nb x 32 | nb x 8
  const void *v_blinding;
  void *proof_points, *proof_scalars, *wire, *challenges_out, *states_out, *gadget_challenges_out;
};
BPGPU_HIDDEN int bpgpu_internal_prove_fs2_chains(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                                 const bpgpu_internal_fs2 &io, int (*between)(void *user, const void *chi_dev), void *user);
// The stages of bpgpu_r1cs_prove_values beside the two above (mutex held, arguments checked, nb > 0, every pointer HBM; asynchronous):
// the refusals of bpgpu_r1cs_prove_fs and of bpgpu_r1cs_commit_values that depend on shapes alone, and the launches of
// bpgpu_r1cs_commit_values_dev, bpgpu_r1cs_constraints_satisfied_dev (no residuals) and bpgpu_r1cs_prove_fs_dev.  _rows_fit builds the
// row-major view of c if it does not exist yet (the one wait of the call) and gives the check's BPGPU_E_LEN before anything else runs.
struct bpgpu_internal_fs1 {
  const void *states_in, *a_L, *a_R, *a_O, *s_L, *s_R, *vector_keys, *v_blinding, *blindings;
  void *proof_points, *proof_scalars, *wire, *challenges_out, *states_out;
};
BPGPU_HIDDEN int bpgpu_internal_prove_fs_shape(const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb);
BPGPU_HIDDEN int bpgpu_internal_commit_values_shape(size_t nb, size_t m);
BPGPU_HIDDEN int bpgpu_internal_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const void *v, const void *v_blinding,
                                              const void *states_in, void *V, void *V_compressed, void *states_out);
BPGPU_HIDDEN int bpgpu_internal_rows_fit(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb);
BPGPU_HIDDEN int bpgpu_internal_constraints_satisfied(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const void *a_L, const void *a_R,
                                                      const void *a_O, const void *v, const void *gadget_challenges, void *ok,
                                                      void *first_bad_row, void *first_bad_gate);
BPGPU_HIDDEN int bpgpu_internal_prove_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const bpgpu_internal_fs1 &io);
// The operands of bpgpu_r1cs_prove_values in the header's order, and its refusals that precede a launch (BPGPU_OK with nb == 0:
// nothing to do): bpgpu_pool.hip asks before it wakes a worker.  Only the handles' shapes and the pointers' presence are read.
struct bpgpu_internal_pv {
  const void *init_states;
  const uint8_t *gadget_label;                                                  // host memory in every form
  const void *v, *v_blinding, *inputs, *s_L, *s_R, *vector_keys, *blindings;
  void *V, *V_compressed, *ok, *first_bad_row, *first_bad_gate, *proof_points, *proof_scalars, *wire, *challenges_out, *states_out,
      *gadget_challenges_out, *a_L_out, *a_R_out, *a_O_out;
};
BPGPU_HIDDEN size_t bpgpu_internal_witness_inputs(const bpgpu_witness *w);      // INPUT pairs per prover
BPGPU_HIDDEN int bpgpu_internal_prove_values_check(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                                                   const bpgpu_internal_pv &a);
#endif
