// kernels.h -- host-callable launchers of the HIP kernels (the k_*.hip files; each section below names its file).
// All pointers are device pointers; every launcher enqueues on `st` and returns immediately.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bpk {

struct JacRaw { int32_t v[27]; };   // unpacked Jacobian limbs (X[9] Y[9] Z[9]), device scratch format
struct AffDev { uint32_t w[16]; };  // packed Montgomery affine (x[8] y[8]); zeros = identity
struct Words8 { uint32_t w[8]; };   // one 256-bit field element (plain canonical at the boundary)

// ---- points ------------------------------------------------------------------------------------
// boundary bytes -> device affine; sets *bad (int) to 1 on a non-canonical / off-curve point
// bad_unit (optional, zeroed by the caller): [i / per_unit] = 1 for a malformed point i (per-proof attribution)
void points_from_boundary(hipStream_t st, const Words8 *xy /*2 per point*/, AffDev *out, size_t n, int *bad,
                          int32_t *bad_unit = nullptr, size_t per_unit = 1);
// out = sum of n boundary points (validated; *bad |= 1 on a malformed one, which is skipped)
void points_sum(hipStream_t st, const Words8 *xy, size_t n, Words8 *out_xy, int *bad);
// JacRaw -> boundary bytes (one inversion per point)
void jac_to_boundary(hipStream_t st, const JacRaw *in, Words8 *xy_out, size_t n);
// JacRaw[n] -> device affine, Montgomery's trick in runs of `run` points per lane
void batch_normalize(hipStream_t st, const JacRaw *in, AffDev *out, size_t n, int run);

// out[i] = sum_{j<np} scalar_j(i) * point_j(i), np in {1..4} (the np points of a lane share one
// doubling chain: ~2 270 + 1 080 np field multiplications per lane instead of 3 350 np).  Two-level indexing for batched
// (proof-major) arrays: i = p * inner + r;
//   point_j(i)  = pts[j] + p * pt_outer[j] + r * pt_stride[j]          (AffDev units)
//   scalar_j(i) = sc[j]  + p * sc_outer[j] + r * sc_stride[j]          (u32 words; stride 0 = broadcast)
// inner == 0 means a flat array (p = 0, r = i).
struct StrausArgs {
  const AffDev *pts[4];
  size_t pt_stride[4];
  const uint32_t *sc[4];
  size_t sc_stride[4];
  size_t inner;
  size_t pt_outer[4];
  size_t sc_outer[4];
  size_t out_outer;   // with inner != 0: out[p * out_outer + r * out_stride]; 0 = dense (out[i])
  size_t out_stride;  // 0 = 1
  int from_boundary;  // pts are ABI bytes (x || y canonical LE words): validate + convert in the kernel, *bad |= 1 on failure
  int *bad;
  int32_t *bad_inner; // optional (zeroed by the caller): [r] = 1 when a point of inner index r (the proof, role-major) is malformed
  int prio;           // fused launch: raise the Straus waves' issue priority
};
// scratch: straus_scratch_bytes(np, n) bytes of device memory private to this launch until it completes
size_t straus_scratch_bytes(int np, size_t n);
void straus(hipStream_t st, int np, const StrausArgs &a, JacRaw *out, size_t n, void *scratch);

// Straus over the proof points (n_lanes lanes) and the small fixed-base MSMs (nb of them) in one launch; false =
// this (np, c, size) combination has no fused kernel, launch the two parts separately
bool verify_msm_fused(hipStream_t st, int np, const StrausArgs &a, JacRaw *out_var, size_t n_lanes, void *scratch, int c,
                      const AffDev *table, size_t n, size_t cap, const uint32_t *scalars, size_t sc_stride_words,
                      JacRaw *out_fixed, size_t nb);

// Window-parallel variant of the same (k_ec.hip): front [tables | inversion pass] -> (k_verify_scalars) -> windows -> groups ->
// back [Horner | fixed-base MSMs] -> verdict, which writes ok / mega itself (no verify_finalize).
// bad_sc: the per-proof canonicity bits written by verify_scalars (nullable)
// latency_mode: more, shorter lanes in the two longest launches (1 point per table lane, 32 lanes per fixed-base MSM, a quad per group in the first Horner stage): one batch
// alone finishes ~25 % sooner, a pipelined stream of batches runs ~5 % slower (more instructions)
// points_converted: points_abi holds AffDev rows (already validated and in Montgomery form: points_from_boundary) instead of ABI bytes
// table_np: points per table lane (1, 2, 4, 8; 0 = by mode: 1 in latency mode, else 8 from 256 proofs on and 4 below) -- BPGPU_OPT_TABLE_NP
struct VerifyWp { const AffDev *points_abi; size_t nb, nvar; void *scratch /* verify_wp_scratch_bytes */; int *bad; const int32_t *bad_sc; bool latency_mode; bool points_converted = false; int table_np = 0;
                  int horner_form = 0;   // Horner pass: 0 = by mode (k_ec.hip: wp_horner_form), 1 = a lane, 2 = a DPP quad, 3 = a wave (row form, ec29_row.cuh) per proof -- BPGPU_OPT_HORNER_FORM
                  size_t row_max = 1536; // most proofs / groups for which latency mode takes the row form -- BPGPU_OPT_HORNER_ROW_MAX
                  int fixed_lpm = 0;     // lanes per fixed-base MSM in the back launch: 16 / 32 / 64, 0 = by mode -- BPGPU_OPT_FIXED_LPM
                  int groups_form = 0;   // first Horner stage: 0 = by mode, 1 = a lane, 2 = a quad, 3 = a wave per group of windows -- BPGPU_OPT_GROUPS_FORM
                  int fixed_chunk_gens = 0;   // generator half of the back launch: 0 = by mode, -1 = fixed_lpm lanes per proof + butterfly; g > 0 = a proof per lane, g generators per wave, partial sums added in the verdict launch -- BPGPU_OPT_FIXED_CHUNK_GENS
                  int horner_group = 0;  // windows per group of the first Horner stage: 8 / 16 / 32, 0 = by mode -- bpgpu_set_horner_group
};
struct VerifyDims { size_t nb, n1, n, padded_n, k, m; const Words8 *chi; /* nb x nchi gadget challenges (plain words) or nullptr */
                    size_t vs_large_min = 0; /* padded_n / m from which the scalar assembly is split over the grid (0 = 4096) -- BPGPU_OPT_VS_LARGE_MIN */ };
struct VsPrepArgs;
size_t verify_wp_scratch_bytes(size_t nb, size_t nvar);
bool verify_wp_supported(size_t nb, size_t nvar, int c, size_t n);
// the launches below carve v.scratch up by (nb, nvar, table_np): true when that layout stays inside verify_wp_scratch_bytes(nb, nvar).
// The caller checks it once after sizing the buffer and fails the call (BPGPU_E_DEVICE) otherwise -- an internal sizing bug must
// not become an out-of-bounds write on the device, nor end the host process.
bool verify_wp_layout_fits(const VerifyWp &v);
// prep_* describe the inversion pass to fuse (vs_prep.cuh; prep_nb == 0: tables only)
// fast_* (all set): the inversion pass also does the serial part of a wave-sized proof's scalar assembly (vs_prep.cuh)
void verify_wp_front_launch(hipStream_t st, const VerifyWp &v, const VerifyDims &d, const Words8 *challenges, int32_t *aux,
                            size_t aux_stride, bool with_prep, const Words8 *fast_proof_scalars = nullptr, Words8 *fast_fixed_sc = nullptr,
                            Words8 *fast_var_sc = nullptr, Words8 *fast_full_sc = nullptr);
void verify_wp_windows(hipStream_t st, const VerifyWp &v, const uint32_t *var_scalars);
void verify_wp_groups(hipStream_t st, const VerifyWp &v);
void verify_wp_back(hipStream_t st, const VerifyWp &v, int c, const AffDev *table, size_t n, size_t cap,
                    const uint32_t *fixed_scalars, size_t sc_stride_words, JacRaw *out_fixed);
// `parts` partial sums of the generator half per proof in `fixed` (verify_wp_fixed_parts: 1 unless v.fixed_chunk_gens > 0 AND the generator
// half rode in verify_wp_back; out_fixed of verify_wp_back must then hold nb x parts entries)
size_t verify_wp_fixed_parts(const VerifyWp &v, size_t n);
void verify_wp_verdict(hipStream_t st, const VerifyWp &v, const JacRaw *fixed, int32_t *ok, Words8 *mega, size_t parts = 1);
// window sums of v's instances (v.nb = v2.nb * per consecutive ones per MSM) added up into v2's window sums: verify_wp_groups / _back then run on v2
void verify_wp_reduce_instances(hipStream_t st, const VerifyWp &v, const VerifyWp &v2, size_t per);
const JacRaw *verify_wp_varsum(const VerifyWp &v);   // nb sums of the proof-point halves, valid after verify_wp_back

// bucket-method MSM of one large instance: out = sum_i scalars[i] * pts[i]   (k_pip.hip)
int pippenger_window(size_t n);
size_t pippenger_scratch_bytes(size_t n, int c);
void pippenger(hipStream_t st, const AffDev *pts, const uint32_t *scalars, size_t n, int c, JacRaw *out, void *scratch);
// ninst independent instances of n terms each (instance-major arrays); out[inst * out_stride]
size_t pippenger_scratch_bytes_batch(size_t ninst, size_t n, int c);
void pippenger_batch(hipStream_t st, const AffDev *pts, const uint32_t *scalars, size_t ninst, size_t n, int c, JacRaw *out,
                     size_t out_stride, void *scratch);
// The launch route of pippenger_batch(ninst, n, c): EVERY decision between two launch chains is taken here, once, on the host, from
// the shape alone; pippenger_batch and pippenger_scratch_bytes_batch read it, and bpgpu_pippenger_plan shows it to the tests.
struct PipPlan {
  int c, W, half;               // window bits, windows, buckets per window
  bool two_level;               // LDS-staged two-level counting sort (k_pip_coarse_* + k_pip_fine_sort) | atomic scatter (k_pip_scatter)
  int shift, shift_top;         // two-level: fine bits of the bucket id in the regular windows and in the top one
  size_t tiles, ngh;            // two-level: key tiles per segment, coarse-histogram entries
  int coarse_scan_launches;     // two-level: launches of the scan of the coarse histograms (2 | 3); 0 without that sort
  uint32_t task;                // entries per task of k_pip_bucket_bounded (PIP_TASK | PIP_TASK_MAX)
  bool task_search;             // task table by a lane per task with a binary search (k_pip_taskdesc_search) | by a loop per bucket
  bool sort_tasks;              // tasks sorted by length before the bucket launch
  int scan_launches;            // launches of a scan over the nbk bucket (and task) counts: 2 | 3
  bool window_ab;               // window sums by k_pip_window_a + _b | by k_pip_window (fewer than 64 buckets per window: no c in [8, 16])
  int window_chunks;            // blocks a window's running sum is cut into
  bool final_quad;              // Horner tail with a quad per instance (k_pip_final) | a wave per instance (k_pip_final_row)
  size_t nbk, tot, max_tasks;   // buckets, terms, upper bound of the task count
};
PipPlan pippenger_plan(size_t ninst, size_t n, int c);
// ---- k_pip2.hip: ONE mid-size instance in six launches (+ a front launch from boundary bytes); 2^8 <= n <= 2^18
int pippenger2_window(size_t n);
bool pippenger2_supported(size_t n);
size_t pippenger2_scratch_bytes(size_t n, int c);
void pippenger2(hipStream_t st, const AffDev *pts, const uint32_t *scalars, size_t n, int c, JacRaw *out, void *scratch, int *bad);
void pippenger2_boundary(hipStream_t st, const Words8 *points_xy, const Words8 *scalars, size_t n, int c, Words8 *out_xy,
                         AffDev *pts_tmp, void *scratch, int *bad);
// gather helper: dst[i] = src[idx(i)] for two-level strided sources (IPP round operands -> contiguous MSM inputs)
void gather_points(hipStream_t st, const AffDev *src, size_t src_outer, size_t cnt, size_t nb, AffDev *dst, size_t dst_outer);
void gather_scalars(hipStream_t st, const Words8 *src, size_t src_outer, size_t cnt, size_t nb, Words8 *dst, size_t dst_outer);

// out[b] = sum_{i<n} in[b*n + i]
void segmented_sum(hipStream_t st, const JacRaw *in, JacRaw *out, size_t nb, size_t n);

// ---- arkworks in-memory forms (k_ark.hip): Scalar = 4 x u64 limbs of x 2^256 mod n; StarkPoint = Jacobian (X : Y : Z), each
// coordinate 4 x u64 limbs of c 2^256 mod p, identity Z = 0
void scalars_from_ark(hipStream_t st, const Words8 *in, Words8 *out_plain, size_t n, int *bad);
void scalars_to_ark(hipStream_t st, const Words8 *in_plain, Words8 *out, size_t n, int *bad);
// rows[2 i] = v[i], rows[2 i + 1] = v_blinding[i], plain canonical words from ark limbs: the (value, blinding) rows of n Pedersen
// commitments over [B, B_blinding], the operand of fixed_msm with zero vector generators
void commit_value_rows(hipStream_t st, const Words8 *v, const Words8 *v_blinding, Words8 *rows, size_t n, int *bad);
void points_from_ark(hipStream_t st, const Words8 *in /* 3 per point */, JacRaw *out, size_t n, int *bad);
void points_to_ark(hipStream_t st, const JacRaw *in, Words8 *out /* 3 per point */, size_t n);
void aff_to_jacraw(hipStream_t st, const AffDev *in, JacRaw *out, size_t n);

// ---- fixed-base tables -------------------------------------------------------------------------
// table[(g*W + w) * 2^(c-1) + (d-1)] = d * 2^(c*w) * P_g,  W = 252/c + 1
size_t fixed_table_entries(int c, size_t ngens);
void fixed_table_build(hipStream_t st, int c, const AffDev *gens, size_t ngens, AffDev *table,
                       JacRaw *scratch /* >= ngens*W + entries */);
// out[b] = sum_g scalars[b*sc_stride + g*8 ..] * P_g over the generators [B, Bb, G_0..G_{n-1}, H_0..H_{n-1}] of a
// table built for capacity cap >= n, via table lookups (plain canonical scalars, 2 + 2n per MSM).
// partials: scratch of nb * fixed_msm_chunks(c, n, nb) points (NULL: one block per MSM).
// out[i] = scalars[i] * (generator 0 of a c = 16 table), one lane per scalar
void fixed_single16(hipStream_t st, const AffDev *table, const uint32_t *scalars, JacRaw *out, size_t n);
// L / R MSMs of an IPP round over resident generators, compact scalars (k_ipp_gens_scalars)
size_t fixed_msm_ipp_chunks(int c, size_t n0, size_t nmsm);
void fixed_msm_ipp(hipStream_t st, int c, const AffDev *table, size_t n0, size_t cap, size_t cur, const uint32_t *scalars,
                   JacRaw *out, size_t nmsm, JacRaw *partials, bool sum_partials = true /* false: the caller sums the nmsm x chunks partials itself (k_ipp_round_tail) */);
// kinds > 0: the nb MSMs are large, many (>= 64 per class) and come in `kinds` interleaved classes (MSM i is of class i % kinds) whose
// scalars look alike within a class -- a batch's A_I, A_O, S rows: an MSM per lane, a run of generators per wave (k_fixed_msm_m)
size_t fixed_msm_chunks(int c, size_t n, size_t nb, int kinds = 0);
void fixed_msm(hipStream_t st, int c, const AffDev *table, size_t n, size_t cap, const uint32_t *scalars,
               size_t sc_stride_words, JacRaw *out, size_t nb, JacRaw *partials, int lpm = 0 /* lanes per small MSM: 32 = shorter lanes for a launch that is a link of a lone chain; 0 = by batch size */,
               int kinds = 0);

// ---- verification tail -------------------------------------------------------------------------
// per proof: sum of nvar variable-base results + the fixed-base partial; ok = is_identity;
// mega (optional) = boundary affine of the sum
// bad_sc / bad_pt (optional): per-proof malformed-input bits; a proof with one set gets ok = 0
void verify_finalize(hipStream_t st, const JacRaw *var, size_t nvar, const JacRaw *fixed, size_t nb,
                     int32_t *ok, Words8 *mega_xy, const int32_t *bad_sc = nullptr, const int32_t *bad_pt = nullptr);

// ---- scalar field (k_scalar.hip) ---------------------------------------------------------------
void scalars_check(hipStream_t st, const Words8 *in, size_t n, int *bad);   // canonical (< n)?
// the same with per-unit attribution: bad_unit[i / per_unit] = 1 for a non-canonical scalar i (bad_unit zeroed by the caller)
void scalars_check_proof(hipStream_t st, const Words8 *in, size_t n, size_t per_unit, int *bad, int32_t *bad_unit);
void batch_inverse(hipStream_t st, Words8 *io, size_t n, int *bad_zero);
void inner_product(hipStream_t st, const Words8 *a, const Words8 *b, size_t n, Words8 *out, void *scratch);
size_t inner_product_scratch_bytes(size_t n);
void fold_scalars(hipStream_t st, size_t n, const Words8 *u, const Words8 *u_inv, const Words8 *a,
                  const Words8 *b, Words8 *a_out, Words8 *b_out);
void verification_scalars(hipStream_t st, const Words8 *challenges, size_t k, size_t n, Words8 *u_sq,
                          Words8 *u_inv_sq, Words8 *s);
// batched IPP scalar kernels (proof-major arrays of nb x n)
// out[p][i] = x[p*x_outer + i*x_stride] * y[p*y_outer + i*y_stride]  for i < cnt (strides in Words8 units)
void sc_mul_strided(hipStream_t st, size_t nb, size_t cnt, const Words8 *x, size_t x_outer, size_t x_stride,
                    const Words8 *y, size_t y_outer, size_t y_stride, Words8 *out);
// out[p] = <x[p*x_outer .. +cnt), y[p*y_outer .. +cnt)>
void sc_dot_batched(hipStream_t st, size_t nb, size_t cnt, const Words8 *x, size_t x_outer, const Words8 *y,
                    size_t y_outer, Words8 *out, size_t out_stride);
// a'[p][i] = a[p][i] u_p + u_p^-1 a[p][h+i] ; b'[p][i] = b[p][i] u_p^-1 + u_p b[p][h+i]   (in: nb x 2h, out: nb x h)
// IPP over resident generators: L/R MSM scalars over the original generators, and the generator fold as a
// coefficient update (see k_scalar.hip)
void ipp_gens_scalars(hipStream_t st, size_t nb, size_t n0, size_t cur, const Words8 *a, const Words8 *b,
                      const Words8 *cG, const Words8 *cH, const Words8 *cLR, const Words8 *w, Words8 *msc, size_t slo = 0,
                      size_t shi = (size_t)-1, bool with_q = true);
void ipp_r1cs_factors(hipStream_t st, size_t nb, size_t np, size_t n1, const Words8 *u, const Words8 *y_inv, Words8 *cG,
                      Words8 *cH);
void ipp_gens_fold(hipStream_t st, size_t nb, size_t n0, size_t cur, const Words8 *u, const Words8 *u_inv, Words8 *cG,
                   Words8 *cH);
void fold_scalars_batched(hipStream_t st, size_t nb, size_t h, const Words8 *u, const Words8 *u_inv, const Words8 *a,
                          const Words8 *b, Words8 *a_out, Words8 *b_out);

// x[p][i] *= w[p]  (in place, nb x cnt) ; out[i] = sum_p w[p] * x[p][i]
void sc_scale_rows(hipStream_t st, size_t nb, size_t cnt, Words8 *x, const Words8 *w);
void sc_weighted_colsum(hipStream_t st, size_t nb, size_t cnt, const Words8 *x, const Words8 *w, Words8 *out);

// column-major constraint weights: for output o in [0, 3n + m + 1): terms col_ptr[o]..col_ptr[o+1]
// outputs ordered wL[0..n) wR[0..n) wO[0..n) wV[0..m) wc
struct CircuitDev {
  const uint32_t *col_ptr;   // 3n + m + 2
  const uint32_t *row;       // nnz: constraint row of the term
  const Words8 *coeff;       // nnz: Montgomery form
  size_t q, n, m, nnz;
  // Randomized (second-phase) constraints whose coefficients are affine in gadget challenges chi_1..chi_nchi (verifier.rs:366-385):
  // a term's row index r' = j * q + r selects the multiplier chi_j (chi_0 = 1) of z^(r+1); the z-power table of a proof then has
  // qz = (1 + nchi) * q entries, zpow[j * q + r] = chi_j * z^(r+1), and the flattening itself is unchanged.
  size_t nchi, qz;
};
// CSR constraint rows (device copies of the ABI arrays; coefficients plain canonical or, ark, ark-ff Montgomery limbs) -> the
// column-major form above: col_ptr (3n + m + 2), rows / coeff_out (nnz, Montgomery form); fill: 3n + m + 1 scratch counters;
// *bad |= 1 on an unknown variable kind, an index out of range or a non-canonical coefficient
void circuit_transpose(hipStream_t st, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx, const Words8 *coeff_in,
                       size_t n_mul, size_t m, bool ark, uint32_t *col_ptr, uint32_t *fill, uint32_t *rows, Words8 *coeff_out, int *bad);
// zpow scratch: nb * q field elements (9 int32 each)
void flatten(hipStream_t st, const CircuitDev &c, size_t nb, const Words8 *z, size_t z_stride_words,
             Words8 *wL, Words8 *wR, Words8 *wO, Words8 *wV, Words8 *wc, int32_t *zpow_scratch, const Words8 *chi = nullptr);

// ---- constraint rows against witnesses (k_rows.hip): Prover::constraints_satisfied (prover.rs:405-409) -------------------------
// The row-major view of a resident circuit: constraint r holds the terms row_ptr[r] .. row_ptr[r + 1], in whatever order the
// scatter left them (the sums are exact in F_n).  Term t: coeff[t] (a COPY of the column-major coefficient, Montgomery form: a row's
// coefficients lie next to each other) and var[t] = idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT -- the variable (kind 0..4 =
// a_L a_R a_O v One, as the CSR of bpgpu_circuit_create) and the gadget challenge chi_j that scales the term (j = 0: none).
// long_rows: the nlong rows of more than rows_lane_max() terms, which a wave evaluates instead of a lane.
constexpr uint32_t ROWS_KIND_SHIFT = 25, ROWS_CHI_SHIFT = 28, ROWS_IDX_MASK = (1u << ROWS_KIND_SHIFT) - 1;
struct RowsDev {
  const uint32_t *row_ptr;   // q + 1
  const uint32_t *var;       // nnz
  const Words8 *coeff;       // nnz
  const uint32_t *long_rows; // nlong
  size_t q, nnz, nlong;
};
uint32_t rows_lane_max();    // a row of up to this many terms is one lane's, a longer one a wave's
bool rows_view_supported(const CircuitDev &c);          // n, m below 2^25 (the packing of var)
size_t rows_view_bytes(const CircuitDev &c);
// builds the view of c in mem (rows_view_bytes, 256-byte aligned); *nlong_dev: where the number of long rows lands (inside mem):
// the caller reads it once the stream has drained and sets view->nlong
void rows_view_build(hipStream_t st, const CircuitDev &c, void *mem, RowsDev *view, const uint32_t **nlong_dev);
// e[p][r] for nvirt provers (planes == 3: virtual prover 3 p + k is plane k of proof p, and a `One` term reads 1 on plane 2 only).
// Operands: plain canonical planes nvirt x n (a_*), nvirt x m (v); chi: nvirt / planes x nchi plain words or nullptr.
// bad_row (optional): nvirt words, atomicMin of the rows with e != 0 (set to 0xFFFFFFFF by the caller); resid (optional): nvirt x q
// plain canonical words.  rows_eval_fits: the grid is addressable
bool rows_eval_fits(const RowsDev &v, size_t nvirt);
void rows_eval(hipStream_t st, const RowsDev &v, size_t n, size_t m, size_t nchi, size_t nvirt, int planes, const Words8 *aL,
               const Words8 *aR, const Words8 *aO, const Words8 *vv, const Words8 *chi, uint32_t *bad_row, Words8 *resid);
// bad_gate[p] = atomicMin of the multipliers i with a_L[i] a_R[i] != a_O[i]
void rows_gates(hipStream_t st, size_t nb, size_t n, const Words8 *aL, const Words8 *aR, const Words8 *aO, uint32_t *bad_gate);
// ok[p] = both words untouched; first_row / first_gate (optional): the word, or -1
void rows_verdict(hipStream_t st, size_t nb, const uint32_t *bad_row, const uint32_t *bad_gate, int32_t *ok, int64_t *first_row,
                  int64_t *first_gate);
// the scan of circuit_transpose on its own (k_scalar.hip k_csr_scan): cnt[0] = 0, cnt[i + 1] = count of i -> cnt[i + 1] = end of i
void csr_scan(hipStream_t st, uint32_t *cnt, size_t n1);

// ---- witness synthesis (k_witness.hip): Prover::multiply / allocate_multiplier (prover.rs:99-125, :148-165) ---------------------
// A resident gate program (bpgpu_witness): gate i owns rows 2 i (left) and 2 i + 1 (right) of `rows` (terms as in a circuit's row-major
// view: Montgomery coefficients, var = idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT; long_rows unused), op[i], arg[i] (the bit of
// a BIT gate, the pair index of an INPUT gate).  The gates of phase ph are listed level by level in order[]: level l of the program
// (phase 1's levels first) holds order[level_ptr[l] .. level_ptr[l + 1]), the gates without a long row (witness_dev.cuh) before
// level_long[l], the others from it.  Validated on the host: every index a kernel forms from these arrays is in range.
// The scan form reads a second set of lists over COMPRESSED levels (bpgpu.h "product chains"): a chain member -- a MUL gate with one
// row that is a single a_O term of its own phase (the link row) and one that reads no multiplier of its phase (the free row) -- takes
// the level of the gate it links to.  Compressed level l holds the ordinary gates scan_order[scan_ptr[l] .. scan_ptr[l + 1]) (heads
// of chains among them; short rows before scan_long[l]) and the members chain_elem[chain_ptr[l] .. chain_ptr[l + 1]) of the chains
// whose head it holds, chain after chain in chain order: gate | WIT_ELEM_START (the first member of a chain) | WIT_ELEM_RIGHT (the
// link is the right row).  Gate ids are below 2^25 (ROWS_IDX_MASK), so the flags are free bits.
// A phase that has AFFINE members (bpgpu.h: the link row holds c a_O[pred] and beside it terms that read nothing of the phase) lists
// the extended chains, product and affine members alike, over the extended compressed levels; an affine member carries
// WIT_ELEM_AFFINE, and its link term stands FIRST in the library's copy of its link row, where wit_link reads it.  Such a phase is
// launched as k_witness_scan<true> (witness_eval's form 4); a phase without one has the lists and the kernel of the product chains alone.
constexpr uint32_t WIT_ELEM_START = 1u << 25, WIT_ELEM_RIGHT = 1u << 26, WIT_ELEM_AFFINE = 1u << 27;
struct WitDev {
  RowsDev rows;
  const uint8_t *op;          // n
  const uint32_t *arg;        // n
  const uint32_t *order;      // n
  const uint32_t *level_ptr;  // levels + 1
  const uint32_t *level_long; // levels
  const uint32_t *scan_order; // n - members
  const uint32_t *scan_ptr;   // compressed levels + 1
  const uint32_t *scan_long;  // compressed levels
  const uint32_t *chain_elem; // members
  const uint32_t *chain_ptr;  // compressed levels + 1
  uint32_t n, m, nchi, ninp;
  // the two-party form (k_mpc_witness.hip) numbers the gates of a level by ascending gate index: asc[level_ptr[l] + t] is the t-th
  // of them, slot[u] the t of order[u]
  const uint32_t *slot;       // n
  const uint32_t *asc;        // n
  // the INV gates (witness_dev.cuh) without a long row stand LAST among a level's short-row gates: order[level_inv[l] ..
  // level_long[l]), and scan_order[scan_inv[l] .. scan_long[l]) of a compressed level; a level without one has level_inv[l] ==
  // level_long[l] and the order it had before the op existed.  Read by the <.., true> instantiations alone.
  const uint32_t *level_inv;  // levels
  const uint32_t *scan_inv;   // compressed levels
};
// One launch evaluates the gates [g_lo, g_hi) = the levels [l_lo, l_hi) of nb provers on plain canonical planes nb x n (aL, aR, aO:
// read for the gates below g_lo, written for the range), v nb x m, inputs nb x ninp x 2, chi nb x nchi (or nullptr), all plain.
// form 1: a lane per prover, program order; 2: a block of 256 threads per prover, level by level; 3: a block per prover over the
// COMPRESSED levels [l_lo, l_hi), the chains of a level as one segmented prefix product (k_witness_scan<false>) or, where the range
// holds an affine member (form 4), as one segmented prefix composition of affine maps (k_witness_scan<true>).
// inv: the range holds an INV gate -- the <.., true> instantiation of the form's kernel, which carries the field inversion (one per
// gate in form 1 and for a long row, one per thread and level otherwise); a range without one launches the kernel it always did.
// div: the range holds a DIVREM gate -- the instantiation that carries the integer division (int_div.cuh), chosen the same way.
void witness_eval(hipStream_t st, const WitDev &w, size_t nb, int form, bool inv, bool div, uint32_t g_lo, uint32_t g_hi, uint32_t l_lo,
                  uint32_t l_hi, Words8 *aL, Words8 *aR, Words8 *aO, const Words8 *v, const Words8 *inputs, const Words8 *chi);
// rows of `count` scalars, one per prover: src + p * src_stride -> dst + p * dst_stride.  to_ark: plain canonical -> ark Montgomery
// limbs, else the reverse; a non-canonical source raises *bad and gives zero
void witness_convert(hipStream_t st, bool to_ark, size_t nb, size_t count, const Words8 *src, size_t src_stride, Words8 *dst,
                     size_t dst_stride, int *bad);

// ---- R1CS prover polynomials (r1cs/prover.rs:587-619, 659-672) -----------------------------------
// polys: raw Montgomery limbs, layout [6][nb][n][9]: l1 l2 l3 r0 r1 r3
void prover_polys(hipStream_t st, const CircuitDev &c, size_t nb, const Words8 *y, const Words8 *y_inv,
                  const Words8 *a_L, const Words8 *a_R, const Words8 *a_O, const Words8 *s_L, const Words8 *s_R,
                  const int32_t *zpow, int32_t *polys, Words8 *wV_out);
// t[nb][6] = t1..t6 (util.rs:152-170 special_inner_product)
void prover_tcoeffs(hipStream_t st, size_t nb, size_t n, const int32_t *polys, Words8 *t_out);
// l_vec, r_vec[nb][padded_n] = l(x), r(x) with the padding of prover.rs:661-672
void prover_eval(hipStream_t st, size_t nb, size_t n, size_t padded_n, const Words8 *x, const Words8 *y,
                 const int32_t *polys, Words8 *l_vec, Words8 *r_vec);
// zpow[b][j * q + r] = chi_{b,j} * z_b^(r+1), j <= nchi (chi: nb x nchi plain words, may be nullptr when nchi = 0)
void zpow_table(hipStream_t st, size_t nb, size_t q, const Words8 *z, size_t z_stride_words, int32_t *zpow, size_t nchi = 0,
                const Words8 *chi = nullptr);

// ---- device-side verifier transcript (k_transcript.hip) ------------------------------
struct TrStep { uint8_t kind, label, validate, pad; uint32_t src; uint64_t value; };
size_t transcript_schedule_max(size_t m, size_t k, size_t nchi = 0);
int transcript_schedule(TrStep *out, size_t m, size_t k, size_t padded_n, size_t nchi = 0);   // host: fills the step list, returns its length
                                                                                                // (nchi > 0: two-phase circuit with nchi gadget challenges)
// A gadget label is 32 bytes, zero-padded; a label TABLE is nchi of them in draw order, resident in HBM at an 8-byte aligned address
// (the callers upload it behind the step list, in the same allocation: gadget_label_slots steps' room).
constexpr size_t GADGET_LABEL_BYTES = 32;
constexpr size_t gadget_label_slots(size_t nchi) { return nchi * GADGET_LABEL_BYTES / sizeof(TrStep); }
// chi_out (nb x nchi): the challenges of the second-phase gadgets.  Draw j hashes under gadget_labels_dev[j] (a label table), or, with
// no table, under gadget_label (host memory; schedule built with nchi = 1)
void verify_transcript(hipStream_t st, size_t nb, size_t m, size_t k, const TrStep *steps_dev, int nsteps, const Words8 *init_state,
                       const Words8 *points, const Words8 *scalars, Words8 *challenges, int32_t *tr_bad,
                       const uint8_t *gadget_label = nullptr, Words8 *chi_out = nullptr, size_t nchi = 0,
                       const uint8_t *gadget_labels_dev = nullptr);
// the same for the segments of ONE mixed check in one launch (nseg <= MIX_SEG_MAX, host array): segment s replays nb proofs of
// (m, k, nchi) on its own schedule (steps_dev, nsteps: resident in HBM), arrays and gadget label (host memory, or null) or label
// table (HBM, or null)
struct TrSegIn {
  const TrStep *steps_dev; int nsteps; size_t nb, m, k, nchi;
  const Words8 *init_state, *points, *scalars; Words8 *challenges, *chi; int32_t *tr_bad; const uint8_t *gadget_label;
  const uint8_t *gadget_labels_dev;
};
void verify_transcript_ragged(hipStream_t st, const TrSegIn *seg, size_t nseg);
void and_not(hipStream_t st, int32_t *ok, const int32_t *bad, size_t n);
void or_flag(hipStream_t st, const int32_t *bad, size_t n, int *flag);
void zero_flag(hipStream_t st, const Words8 *s, size_t n, int *flag);

// Verifier scalar assembly (r1cs/verifier.rs:457-532).  Writes
//   fixed_sc[nb][2 + 2*padded_n] (B, B_blinding, g, h) and var_sc[nb][11 + m + 2k]
//   (A_I1 A_O1 S1 A_I2 A_O2 S2 V.. T_1 T_3 T_4 T_5 T_6 L.. R..), plain canonical words;
//   full_sc (optional): nb x (13 + m + 2 padded_n + 2k) in verifier.rs:517-532 order.
//   bad (optional): set to 1 when a challenge or proof scalar is not canonical (< n)
//   zpow_scratch: verify_scalars_scratch_ints(c, d) int32 (z powers + the large-proof path's partials)
size_t verify_scalars_scratch_ints(const CircuitDev &c, const VerifyDims &d);
//   bad_proof (optional): nb int32, [p] = 1 when one of proof p's challenges / scalars is not canonical, else 0
//   prep_done: the inversion pass (vs_prep.cuh) has already run into the aux area of zpow_scratch (verify_scalars_aux)
void verify_scalars(hipStream_t st, const CircuitDev &c, const VerifyDims &d, const Words8 *challenges,
                    const Words8 *proof_scalars, Words8 *fixed_sc, Words8 *var_sc, Words8 *full_sc,
                    int32_t *zpow_scratch, int *bad, int32_t *bad_proof = nullptr, bool prep_done = false, bool prep_fast = false);
// wave-sized proofs (padded n = 64): the inversion pass can also do the serial part of the assembly when it is given the proof
// scalars and the output arrays (vs_prep.cuh); prep_fast tells verify_scalars that the caller's fused launch has done so
bool verify_scalars_fast_shape(const CircuitDev &c, const VerifyDims &d);
// where the inversion pass writes (inside zpow_scratch) and its per-proof stride in field elements; false = the large-proof
// path, which runs its own inversion pass
bool verify_scalars_aux(const CircuitDev &c, const VerifyDims &d, int32_t *zpow_scratch, int32_t **aux, size_t *aux_stride);

// ---- combined batch check in eight launches (k_pip2.hip): sum_p rho_p * mega_check_p as ONE boundary point
// optional stage markers for per-kernel event timing: fn(ctx, kind, stream) is called before and after a stage
typedef void (*ProfMarkFn)(void *ctx, int kind, hipStream_t st);
struct ProfMark {
  ProfMarkFn fn; void *ctx; int kind; hipStream_t st;
  ProfMark(ProfMarkFn f, void *c, int k, hipStream_t s) : fn(f), ctx(c), kind(k), st(s) { if (fn) fn(ctx, kind, st); }
  ~ProfMark() { if (fn) fn(ctx, kind, st); }
};
struct CombinedArgs {
  CircuitDev circ; VerifyDims d; size_t nvar;
  const Words8 *points, *proof_scalars, *challenges, *rho;     // ABI bytes in HBM
  Words8 *fixed_sc, *var_sc;                                   // nb x (2 + 2 padded_n), nb x nvar (written here)
  int32_t *zpow_scratch;                                       // verify_scalars_scratch_ints
  const AffDev *table; size_t cap; int c;                      // resident generator tables
  void *scratch;                                               // verify_combined2_scratch_bytes
  int *bad; Words8 *partial_xy;                                // out: 64 boundary bytes
  ProfMarkFn prof; void *prof_ctx;
};
size_t verify_combined2_scratch_bytes(size_t nb, size_t nvar, size_t nfix);
bool verify_combined2_supported(size_t nb, size_t nvar, int c, size_t padded_n);
void verify_combined2(hipStream_t st, const CombinedArgs &a);

// ---- ragged combined check (k_mixed.hip): sum_p rho_p * mega_check_p over proofs of SEVERAL circuits as ONE boundary point.
// A segment is a run of consecutive proofs of one circuit; a check holds up to MIX_SEG_MAX of them.  The generator half sums into
// the common layout [B, B_blinding, G_0..G_{N-1}, H_0..H_{N-1}], N = the largest padded n of the check's segments.
constexpr size_t MIX_SEG_MAX = 16;
struct MixSegIn {
  CircuitDev circ; VerifyDims d;     // d.nb = the segment's proofs; d.chi = their gadget challenges (nb x nchi) or nullptr
  size_t nvar, nchi;
  const Words8 *points, *proof_scalars, *challenges, *rho;   // ABI bytes in HBM, from the segment's first proof on
};
struct MixedArgs {
  const MixSegIn *seg; size_t nseg;  // host array, nseg <= MIX_SEG_MAX
  void *scratch;                     // verify_mixed_scratch_bytes
  const AffDev *table; size_t cap; int c;   // resident generator tables
  int *bad;                          // malformed point, non-canonical scalar / challenge / gadget challenge / weight
  int *zero_rho;                     // optional: set when a weight is zero (the screened call voids such a check)
  Words8 *partial_xy;                // out: 64 boundary bytes
  ProfMarkFn prof; void *prof_ctx;
};
size_t verify_mixed_scratch_bytes(const MixSegIn *seg, size_t nseg, int c /* the generator tables' window */);
// front, one scalar assembly per segment, K1 and the k_pip2.hip tail (profiling slots 12, 13, 15) when the check fits the
// one-instance bucket pipeline; otherwise the same front and column sum, then k_fixed.hip's and k_pip.hip's MSMs (all on `st`)
void verify_mixed(hipStream_t st, const MixedArgs &a);
// *bad != 0: out_xy := 64 bytes 0xFF (not a point; bpgpu_points_sum rejects it) -- the combined entry points' verdict on malformed input
void mixed_poison(hipStream_t st, const int *bad, Words8 *out_xy);

// the prover's blinding vectors drawn on the device from per-prover keys (k_transcript.hip, "BlindVec v1"):
// sL / sR [p * stride + off + i] for i < cnt, plain canonical words
void blind_vectors(hipStream_t st, const Words8 *keys, size_t nb, size_t cnt, Words8 *sL, Words8 *sR, size_t stride, size_t off);
// MSM scalar rows of the three commitments A_I, A_O, S of nb provers over [B, B_blinding, G_0.., H_0..] (prover.rs:465-494 /
// :532-565): rows[(3 p + w) * (2 + 2 n)] for w = 0, 1, 2 from the witness planes (nb x stride, plain canonical; multipliers
// [lo, n) are live, the rest of a row is zero) and blinds (nb x 3: i, o, s blinding)
// [slo, shi): the generator indices of THIS rank's share when one large proof is split over the GPUs of a node (the other
// entries of a row are zero; with_blind: the B_blinding term belongs to one rank only); default = everything
void commit_rows(hipStream_t st, size_t nb, size_t n, size_t lo, size_t stride, const Words8 *aL, const Words8 *aR, const Words8 *aO,
                 const Words8 *sL, const Words8 *sR, const Words8 *blinds, Words8 *rows, size_t slo = 0, size_t shi = (size_t)-1,
                 bool with_blind = true);
void shard_mask(hipStream_t st, Words8 *fixed, size_t np, size_t slo, size_t shi, bool keep_pedersen, Words8 *var, size_t nvar, size_t vlo,
                size_t vhi);
// one IPP prover round of the device transcript: append L, R; u = challenge (k_transcript.hip)
void ipp_round_challenge(hipStream_t st, size_t nb, uint64_t *states, const Words8 *lr_xy, Words8 *u_out);
// the whole tail of a round in one launch: L, R (Jacobian sums, nb x 2) -> boundary bytes, the three transcript steps on a
// wave-cooperative Keccak, u and u^-1
void ipp_round_tail(hipStream_t st, size_t nb, const JacRaw *sums, uint64_t *states, Words8 *lr_xy, Words8 *u_out, Words8 *uinv_out, const JacRaw *partials = nullptr, size_t chunks = 0 /* > 1: sums[2p + s] = sum of partials[(2p + s) * chunks + i], added up here */);

// ---- the one-call prover (bpgpu_r1cs_prove_fs): the prover's transcript slices (k_transcript.hip) and the links between the stages
// (k_prove_fs.hip) ------------------------------------------------------------------------------------
// host: the prover's step list and its slices, slice j = steps [cut[j], cut[j + 1]).  A one-phase circuit: 22 steps in three slices,
// up to y, z | T points, u, x | t_x t_x_blinding e_blinding, w, the IPP separator.  A two-phase circuit with nchi <= 8 gadget
// challenges (nchi = 0: one phase): 23 + nchi steps in four, up to the last gadget challenge | A_I2 A_O2 S2, y, z | then the same two
constexpr int PROVER_SCHEDULE_MAX = 32;
int prover_transcript_schedule(TrStep *out, size_t nchi, size_t m, size_t padded_n, int cut[5]);
// one slice for nb provers, a lane each; states: 4 x u64 per prover, updated.  A step's src indexes points (pt_stride per prover),
// scalars (sc_stride per prover) or the challenge ARRAYS: challenges[src * nb + p].  TS_GADGET_CHALLENGE step j draws into
// chi[p * nchi + j] under gadget_labels_dev[j] (a label table, as verify_transcript's) or, with no table, under gadget_label (32 bytes,
// zero-padded, host memory)
void prover_transcript(hipStream_t st, size_t nb, const TrStep *steps_dev, int nsteps, uint64_t *states, const Words8 *points,
                       size_t pt_stride, const Words8 *scalars, size_t sc_stride, Words8 *challenges, const uint8_t *gadget_label = nullptr,
                       Words8 *chi = nullptr, size_t nchi = 1, const uint8_t *gadget_labels_dev = nullptr);
// the chain before Prover::prove (bpgpu_r1cs_commit_values), a lane per prover: r1cs_domain_sep, then append_point("V", V_j) over the
// prover's m boundary points (nb x m, prover-major).  states_in / states_out: nb x 32 B, may alias
void commit_transcript(hipStream_t st, size_t nb, size_t m, const Words8 *states_in, const Words8 *points, Words8 *states_out);
// rows[(5 p + j) * 2 ..] = (t, t_blinding) of T_1, T_3..T_6 over [B, B_blinding]; t: nb x 6, bl: nb x 8 (i o s blinding, tb1 tb3 tb4 tb5 tb6)
void prove_fs_t_rows(hipStream_t st, size_t nb, const Words8 *t, const Words8 *bl, Words8 *rows);
// out[p] = (t_x, t_x_blinding, e_blinding) from x, t, bl and tb2 = <wV, v_blinding>: summed by the proof's lane for m up to
// PROVE_FS_DOT_LANE_MAX (tb2_pre = nullptr), above it taken from tb2_pre (nb values of sc_dot_batched, a block per proof)
constexpr size_t PROVE_FS_DOT_LANE_MAX = 16;
// two phases (u, bl1 non-null): bl's first three are the SECOND phase's blinding factors, bl1 (nb x 3) the first's, and
// e_blinding = x ((i1 + u i2) + x ((o1 + u o2) + x (s1 + u s2)))
void prove_fs_glue(hipStream_t st, size_t nb, size_t m, const Words8 *x, const Words8 *t, const Words8 *bl, const Words8 *wV, const Words8 *vb,
                   const Words8 *tb2_pre, Words8 *out, const Words8 *u = nullptr, const Words8 *bl1 = nullptr);
// proof assembly (layouts: k_prove_fs.hip): proof_points, proof_scalars, and the optional wire form, challenges and chain states
struct ProveFsAssemble {
  size_t nb, k;
  const Words8 *A, *T, *lr, *sc3, *a, *b, *ch, *uch;
  const uint64_t *states;
  Words8 *proof_points, *proof_scalars, *challenges_out, *states_out;
  uint8_t *wire;
  const Words8 *A2 = nullptr;   // two phases: nb x 3 points A_I2 A_O2 S2 (nullptr: the identity, wire version 0)
};
void prove_fs_assemble(hipStream_t st, const ProveFsAssemble &a);
// the rows of the provers with ok[p] == 0 cleared to zero bytes (bpgpu_r1cs_prove_values: a rejected prover ships nothing).  Per prover:
// proof_points b_points bytes (a multiple of 64), proof_scalars 160, and the optional challenges_out b_chal (a multiple of 32),
// states_out 32 and wire b_wire (any length); all but wire 4-byte aligned
struct ProveFsClear {
  size_t nb, b_points, b_chal, b_wire;
  const int32_t *ok;
  uint8_t *proof_points, *proof_scalars, *challenges_out, *states_out, *wire;
};
void prove_fs_clear_rejected(hipStream_t st, const ProveFsClear &a);

// ---- two-party prover, one party's local arithmetic (k_mpc.hip): 3 nb virtual provers v = 3 p + k (k = 0 share, 1 MAC, 2 public
// modifier); triples [p][j][x, y, z][k][i], masked [p][j][d, e][k][i], opened [p][j][d, e][i] (plain canonical words)
// polys [6][3 nb][n][9] as prover_polys (r0 holds the public value on every plane); y, y_inv: 3 nb; wV_out: nb x m; j < 6
void mpc_polys(hipStream_t st, const CircuitDev &c, size_t nb, const Words8 *y, const Words8 *y_inv, const Words8 *a_L,
               const Words8 *a_R, const Words8 *a_O, const Words8 *s_L, const Words8 *s_R, const int32_t *zpow, int32_t *polys,
               Words8 *wV_out, const Words8 *trip, Words8 *masked);
// t_out[3 nb][6]: t1..t6 per plane from the Beaver combine of the six products and the local products with r0
void mpc_tcoeffs(hipStream_t st, size_t nb, size_t n, const int32_t *polys, const Words8 *opened, const Words8 *trip, Words8 *t_out);
// rows[(5 v + j) * 2 ..]: [t, t_blinding] of T_1, T_3..T_6 over [B, B_blinding] (t: nvirt x 6, tb: nvirt x 5)
void mpc_t_rows(hipStream_t st, size_t nvirt, const Words8 *t, const Words8 *tb, Words8 *rows);
// l_vec, r_vec[3 nb][padded_n]: l(x), r(x) per plane, r0 and the -y^i padding on the modifier plane (x, y: 3 nb)
void mpc_eval(hipStream_t st, size_t nb, size_t n, size_t padded_n, const Words8 *x, const Words8 *y, const int32_t *polys, Words8 *l_vec,
              Words8 *r_vec);
// IPP round: masked values of c_L = <a_L, b_R>, c_R = <a_R, b_L> (j = 0, 1; a, b: 3 nb x 2h), then their combine into cLR[2 v + j]
void mpc_ipp_mask(hipStream_t st, size_t nb, size_t h, const Words8 *a, const Words8 *b, const Words8 *trip, Words8 *masked);
void mpc_ipp_combine(hipStream_t st, size_t nb, size_t h, const Words8 *opened, const Words8 *trip, Words8 *cLR);

// ---- two-party witness synthesis (k_mpc_witness.hip): MpcProver::multiply / allocate_multiplier (mpc_prover.rs:183-282), one
// dependency level of a gate program per launch pair.  The level is order[lo .. hi) of w, the gates without a long row before mid; it
// has G = hi - lo gates, and slot t is the t-th of them in ascending gate index.  Planes of the 3 nb virtual provers, plain canonical
// words: aL, aR, aO 3 nb x n, v 3 nb x m, inputs 3 nb x ninp x 2; chi nb x nchi (public, per proof; nullptr without);
// trip [p][x, y, z][k][t], masked [p][d, e][k][t], opened [p][d, e][t]: the layouts above with one product per proof, len = G.
struct MpcWitLevel {
  WitDev w;
  size_t nb;
  uint32_t lo, mid, hi;
  Words8 *aL, *aR, *aO;
  const Words8 *v, *inputs, *chi, *trip;
  Words8 *masked;
};
// a_L, a_R of the level's gates on every plane (a `One` term on the modifier plane only), and masked d = a_L - x, e = a_R - y
void mpc_witness_mask(hipStream_t st, const MpcWitLevel &a);
// a_O of the level's gates: z_k + d y_k + e x_k, plus d e on the modifier plane
void mpc_witness_combine(hipStream_t st, const MpcWitLevel &a, const Words8 *opened);

// ---- InnerProductProof::verify for nb proofs of one length n = 2^k (k_ippv.hip) -------------------
// header, a lane per proof: hdr[p] = (k + 2) x 9 int32 (u_j^2, a / prod u, b / prod u: what ippv_assemble reads); the scalars of
// Q (a b, times w[p] when w is given: Q = w B), L_j (-u_j^2) and R_j (-u_j^-2) as plain words at q_sc[p * q_stride],
// l_sc / r_sc[p * lr_stride + j]; zero_sc (optional): [p * q_stride] := 0.  reject[p] = 1 for a zero challenge (writes 1 only);
// *bad |= 1 for a non-canonical challenge, a, b or w.
struct IppvHeader { size_t nb; int k; const Words8 *challenges, *ab, *w; int32_t *hdr; Words8 *q_sc, *zero_sc; size_t q_stride;
                    Words8 *l_sc, *r_sc; size_t lr_stride; int32_t *reject; int *bad; };
void ippv_header(hipStream_t st, const IppvHeader &h);
// g_sc[p * sc_stride + i] = a s_i Gf[p][i], h_sc[p * sc_stride + i] = b s_{n-1-i} Hf[p][i] (s is not stored); *bad |= 1 for a
// non-canonical factor.  ippv_assemble_fits: the launch's grid is addressable
bool ippv_assemble_fits(size_t nb, size_t n);
void ippv_assemble(hipStream_t st, size_t nb, size_t n, size_t k, const int32_t *hdr, const Words8 *Gf, const Words8 *Hf, Words8 *g_sc,
                   Words8 *h_sc, size_t sc_stride, int *bad);
// boundary points -> dst[p * stride + row]: the segments with check_only = 0 fill rows [0, used) in order (segment row q of proof p
// reads src[p * outer + q]; outer = 0: one array for all proofs), rows [used, stride) become identity points and pad_sc there zero
// scalars; check_only segments (`extra` rows per proof in all) are validated and not stored.  *bad |= 1 on a malformed point.
struct IppvSeg { const Words8 *src; size_t outer, cnt; int check_only; };
struct IppvPoints { IppvSeg seg[6]; int nseg; size_t nb, stride, used, extra; AffDev *dst; Words8 *pad_sc; int *bad; };
void ippv_points(hipStream_t st, const IppvPoints &a);
// ok[p] = expect_P[p] == P[p] (64 boundary bytes each) && !reject[p]
void ippv_verdict(hipStream_t st, size_t nb, const Words8 *expect_xy, const Words8 *P_xy, const int32_t *reject, int32_t *ok);
// the verifier's transcript replay (k_transcript.hip; inner_product_proof.rs:269-278 after the domain separator), a lane per
// proof: k x (append_point "L", "R"; challenge_scalar "u").  L, R: nb x k points (proof-major); challenges: nb x k;
// reject[p] = 1 for an identity L or R (validate_and_append_point; writes 1 only); states_out may alias states_in
void ippv_transcript(hipStream_t st, size_t nb, size_t k, const Words8 *states_in, const Words8 *L, const Words8 *R, Words8 *challenges,
                     int32_t *reject, Words8 *states_out);

// ---- wire codec of points (k_codec.hip): 32-byte compressed <-> 64-byte affine boundary form ------
size_t sqrt_table_bytes();
void sqrt_tables_build(hipStream_t st, void *tab /* sqrt_table_bytes() */);
void points_decompress(hipStream_t st, const Words8 *in, Words8 *out_xy, int32_t *ok, size_t n, const void *tab);
void points_compress(hipStream_t st, const Words8 *xy, Words8 *out, size_t n);
// wire-format proofs -> operands of the verification pipeline (k_codec.hip)
void wire_unpack(hipStream_t st, const uint8_t *proofs, size_t proof_len, const uint8_t *commitments, size_t nb, size_t m,
                 size_t k, int two_phase, Words8 *comp, Words8 *scalars, int32_t *fmt_ok);
void wire_and_ok(hipStream_t st, int32_t *ok, const int32_t *fmt_ok, const int32_t *dec_ok, size_t nb, size_t nvar);
// the segments of ONE mixed check (nseg <= MIX_SEG_MAX, host array) in one launch: comp holds the segments' points one after the
// other (nb x nvar each), scalars / fmt_ok go by the check's proof index
struct WireSegIn { const uint8_t *proofs, *commitments; size_t proof_len, nb, m, k; bool two_phase; };
void wire_unpack_ragged(hipStream_t st, const WireSegIn *seg, size_t nseg, Words8 *comp, Words8 *scalars, int32_t *fmt_ok);
// bad[p] = !fmt_ok[p] | any !dec_ok[p][*] | tr_bad[p] (all indexed as wire_unpack_ragged lays them out); *flag |= bit if any is set
void wire_fold(hipStream_t st, const WireSegIn *seg, size_t nseg, const int32_t *fmt_ok, const int32_t *dec_ok, const int32_t *tr_bad,
               int32_t *bad, int *flag, int bit);

}  // namespace bpk
