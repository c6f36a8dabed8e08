/*
 * bpgpu.h -- C ABI of the MI355X-native Bulletproofs hot path (Stark curve).
 *
 * Drop-in boundary for renegade-fi/mpc-bulletproof: the reference has no FFI; its hot path calls
 * free functions of the external crate mpc-stark (Scalar, StarkPoint) at the sites cited below
 * (paths relative to the reference root).  A Rust shim binds these symbols in place of those calls
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - scalar : 32-byte little-endian canonical integer < n (group order).  Non-canonical -> BPGPU_E_ARG.
 *   - point  : affine x || y, 32-byte little-endian canonical each (< p); 64 zero bytes = identity
 *              (the encoding the reference absorbs into the transcript, src/util.rs:274-289).
 *              Off-curve / non-canonical -> BPGPU_E_ARG.
 *   - all pointers are caller-owned; nothing allocated here crosses the boundary except opaque
 *     handles released by the matching *_destroy; functions never throw; return 0 or BPGPU_E_*.
 *   - thread-safe: a bpgpu_ctx may be shared by threads (calls on one ctx are serialised by an
 *     internal mutex; use one ctx per thread for concurrency) -- the reference calls msm from rayon
 *     workers and MPC-fabric executor threads (src/inner_product_proof.rs:233-247, src/transcript.rs:155-161).
 *   - `_dev` variants take device pointers obtained from bpgpu_malloc (or any HIP allocation of the
 *     same device, e.g. a torch tensor's data_ptr) and enqueue on the ctx stream without a host sync.
 *   - no CPU fallback exists: without a usable HIP device every call returns BPGPU_E_DEVICE.
 */
#ifndef BPGPU_H
#define BPGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPGPU_OK 0
#define BPGPU_E_ARG (-1)     /* malformed input: non-canonical scalar, off-curve point, null pointer */
#define BPGPU_E_LEN (-2)     /* length mismatch / not a power of two where required (reference panics: inner_product_proof.rs:62-70) */
#define BPGPU_E_DEVICE (-3)  /* HIP error / no device */
#define BPGPU_E_OOM (-4)
#define BPGPU_E_GENS (-5)    /* generator capacity too small: R1CSError::InvalidGeneratorsLength (verifier.rs:421-423) */

typedef struct bpgpu_ctx bpgpu_ctx;
typedef struct bpgpu_gens bpgpu_gens;       /* resident generators + fixed-base tables */
typedef struct bpgpu_circuit bpgpu_circuit; /* resident constraint weights (column-major) */

/* ---- context ------------------------------------------------------------------------------- */
int bpgpu_device_count(void);
int bpgpu_create(int device, bpgpu_ctx **out);
void bpgpu_destroy(bpgpu_ctx *ctx);
const char *bpgpu_strerror(int code);
const char *bpgpu_last_error(bpgpu_ctx *ctx);   /* text of the last HIP failure on this ctx */
int bpgpu_sync(bpgpu_ctx *ctx);
void *bpgpu_stream(bpgpu_ctx *ctx);             /* hipStream_t of the ctx (for event timing) */
/* Hardware queues.  The pipelined entry points (several contexts driven in turn, the stream, screened and mixed calls, the pool,
 * the host mirror's prover streams) keep ~20 batches in flight on a stream each, and reach their rate only when those streams
 * land on as many hardware queues.  The HIP runtime takes the number from GPU_MAX_HW_QUEUES when it initialises (default 4), so
 * libbpgpu.so claims its requirement of 24 when it is LOADED:
 *   GPU_MAX_HW_QUEUES unset, not a number, or below 24  -> the library exports 24 (an inherited 4 cannot be told from "nobody
 *                                                          chose", and keeping it costs a third to two thirds of the rate);
 *   GPU_MAX_HW_QUEUES at or above 24                    -> left alone (never lowered; the library never exports more than 32);
 *   BPGPU_HW_QUEUES = 1..32                             -> exactly that is exported, over any inherited value;
 *   BPGPU_HW_QUEUES = 0                                 -> the process's setting is left untouched (a host that limits queues
 *                                                          on purpose); any other text is ignored.
 * No other variable of the runtime is read or written.  A process that has initialised HIP before loading the library keeps
 * what the runtime read then.  The getter reports what happened at load (a C setenv is invisible to a snapshot of the environment
 * such as Python's os.environ): *inherited = the value the process environment held, *in_force = the value the library left
 * there; each -1 if unset, -2 if set to something that is not a number (read as the runtime reads it: the leading decimal
 * integer; a negative one reports as 0).  Either pointer may be NULL.  Returns BPGPU_OK. */
int bpgpu_hw_queues(int *inherited, int *in_force);
/* Tuning hint for the batch-verification entry points of this context.  0 (default): fewest instructions -- right for a
 * caller that keeps several batches in flight (several contexts / streams), where throughput is bound by instruction issue.
 * 1: more, shorter lanes in the two longest launches of a batch's kernel chain -- one batch alone completes ~25 % sooner
 * (0.8 instead of 1.05 ms for 1024 x 64-bit range proofs), a saturated pipeline runs ~5 % slower.  Results are identical. */
int bpgpu_set_latency_mode(bpgpu_ctx *ctx, int on);
/* Launch-route options of ONE context (results never depend on them: every route computes the same bytes; the parity tests
 * walk all of them through this setter).  The environment variables BPGPU_<NAME> of the same names only seed a new context's
 * defaults, once, inside bpgpu_create -- nothing reads the environment per call.  BPGPU_E_ARG for an unknown option or a
 * value outside its range. */
#define BPGPU_OPT_MSM_WP_MAX 1             /* MSMs of up to this many terms take the window-parallel launches (default 2^15; 0 = never) */
#define BPGPU_OPT_MSM_PIP2_SINGLE 2        /* 1: one mid-size MSM through k_pip2.hip's one-instance bucket pipeline (default 0) */
#define BPGPU_OPT_VERIFY_NO_FUSE 3         /* 1: verification as separate point-import / Straus / fixed-base / finalize launches (default 0) */
#define BPGPU_OPT_VERIFY_WINDOW_PARALLEL 4 /* 0: the fused Straus + fixed-base launch instead of the window-parallel chain (default 1) */
#define BPGPU_OPT_VERIFY_STRAUS_NP 5       /* points per Straus lane on those paths, 1..4 (default 4) */
#define BPGPU_OPT_IPP_LITERAL 6            /* 1: bpgpu_ipp_begin always runs the reference's literal schedule (generators folded every round) */
#define BPGPU_OPT_VS_LARGE_MIN 7           /* padded n / m from which the verifier's scalar assembly is split over the grid (default 4096) */
#define BPGPU_OPT_TABLE_NP 8               /* proof points per table lane of the window-parallel chain: 1, 2, 4, 8; 0 = by mode (1 in latency mode; 8 for batches of 256 proofs or more -- fewest instructions, a longer launch: see bpgpu_set_horner_group --, 4 below) */
#define BPGPU_OPT_IPP_TABLE_MAX_N 9        /* bpgpu_ipp_begin builds per-session generator tables up to this n (default 2^16), literal schedule above */
#define BPGPU_OPT_STREAM_LANES 10          /* lanes (streams + workspaces) a bpgpu_r1cs_verify_stream call spreads its batches over, 1..64 (default 20) */
#define BPGPU_OPT_STREAM_BATCH 11          /* proofs per batch of a bpgpu_r1cs_verify_stream call (default 1024) */
#define BPGPU_OPT_SCREEN_BATCH 12          /* proofs per combined check of a bpgpu_r1cs_verify_screened call (default 2560; capped so that one check's proof points stay within the one-instance bucket pipeline) */
#define BPGPU_OPT_HORNER_FORM 13           /* Horner pass of the window-parallel chain / MSMs: 0 = by mode, 1 = a lane, 2 = a DPP quad, 3 = a whole wave (row-distributed field arithmetic) per proof / group */
#define BPGPU_OPT_HORNER_ROW_MAX 14        /* latency mode and the MSMs take the wave-per-chain form up to this many chains (default 1536: one wave per SIMD and a half) */
#define BPGPU_OPT_PIPPENGER_MIN 15         /* terms from which an MSM that is not served by the window-parallel launches takes the bucket method (default 512) */
#define BPGPU_OPT_IPP_PIPPENGER_MIN 16     /* the same for the L / R MSMs of bpgpu_ipp_round's literal schedule (default 257) */
#define BPGPU_OPT_FIXED_LPM 17             /* lanes per fixed-base MSM in the verification's back launch: 16, 32, 64; 0 = by mode */
#define BPGPU_OPT_GROUPS_FORM 18           /* first Horner stage: 0 = by mode, 1 = a lane, 2 = a DPP quad, 3 = a whole wave per group of windows (bpgpu_set_horner_group) */
#define BPGPU_OPT_FIXED_CHUNK_GENS 19      /* generator half of the verification's back launch: 0 = by mode, -1 = FIXED_LPM lanes per proof and a butterfly; g in 1..64 = a proof
                                            * per lane, g generators per wave, the partial sums added in the verdict launch */
#define BPGPU_OPT_WITNESS_ROUTE 20         /* witness synthesis (bpgpu_r1cs_witness_synthesize, bpgpu_r1cs_prove_fs2): 0 = by bpgpu_witness_plan and BPGPU_OPT_WITNESS_SCAN_MIN, 1 = a lane per prover, 2 = a block per prover */
#define BPGPU_OPT_WITNESS_SCAN_MIN 21      /* under WITNESS_ROUTE 0, a phase whose longest product chain has this many members or more takes the scan form (default 16; 0 = never; up to 2^25) */
#define BPGPU_OPT_COUNT 22
int bpgpu_set_option(bpgpu_ctx *ctx, int option, int64_t value);
int bpgpu_get_option(bpgpu_ctx *ctx, int option, int64_t *value);
/* Windows per group of the first Horner stage of the window-parallel chain / MSMs (the second stage then takes 64 / this many
 * partial sums per proof): 8, 16 or 32; 0 (default) = by mode: 32 for batches of 256 proofs or more outside latency mode, 8
 * otherwise and in the MSMs.  A launch-route setting of ONE context like the options above -- results never depend on it --
 * with a setter of its own: BPGPU_E_ARG for any other value, which leaves the setting as it was.  The environment variable
 * BPGPU_HORNER_GROUP seeds a new context through the same validation.  Why not a numbered option: BPGPU_OPT_COUNT is pinned at
 * 22 by the ABI tests of the witness entry points (tests/test_witness_chains_abi.py, tests/test_witness_affine_abi.py), and the
 * change that added this setting could not edit them.  A consequence: bpgpu_pool_set_option does not reach it; the slots of a
 * pool get it from the environment only.
 * By mode, a batch of 256 proofs or more outside latency mode takes the shapes with the fewest instructions (this, a lane per
 * proof in the second stage, BPGPU_OPT_TABLE_NP = 8): right for a caller that keeps several batches in flight; ONE such batch
 * alone on the chip is 0.41 ms longer than with the short shapes (1 024 64-bit range proofs) -- use bpgpu_set_latency_mode there. */
int bpgpu_set_horner_group(bpgpu_ctx *ctx, int windows);
int bpgpu_get_horner_group(bpgpu_ctx *ctx, int *windows);
/* synchronise and report whether an operand of the `_dev` (device-resident, asynchronous) calls issued since the last read -- or
 * since the last synchronous entry point on this context, each of which uses and clears the flag for its own BPGPU_E_ARG -- was
 * malformed (1); reading clears the flag.  A diagnostic: the verification entry points reject a malformed proof on its own
 * (ok[p] = 0; that includes a non-canonical gadget challenge of bpgpu_r1cs_verify_batch_param) and never fail the call for it. */
int bpgpu_input_flag(bpgpu_ctx *ctx, int *bad);

/* Per-kernel timing with HIP events recorded on the stream each kernel is launched on (the numbers
 * bench.py's `roofline` uses).  BPGPU_PROF_KINDS kinds.  Window-parallel verification chain (the default):
 * 8 front (proof-point tables | inversion pass), 0 scalar assembly (k_verify_scalars), 7 window sums, 9 Horner
 * groups, 10 back (Horner pass | fixed-base MSMs), 11 verdict; 5 device transcript; 12..15 the stages of the
 * combined batch check (scalars + weights, proof-point MSM, generator MSM, tail).  Other launch paths: 6 fused Straus +
 * fixed-base launch, 1 fixed-base MSM, 2 point import, 3 Straus, 4 verify tail.  read() synchronises, returns sums
 * since the last read (at most 64 launches per kind are kept between two reads).  select() restricts the timing to the
 * kinds of a bit mask (bit k = kind k; default all): an event pair is a barrier in the queue on either side of its kernel,
 * so a caller that wants one kernel's duration out of a pipelined run pays for that kernel only. */
#define BPGPU_PROF_KINDS 24
/* Kinds 16..21 cover the prover (one pair per device phase of a call, i.e. from its first to its last launch): 16 phase commitments
 * (bpgpu_r1cs_prover_commit), 17 polynomial build, 18 bpgpu_msm_gens (T commitments), 19 IPP session set-up, 20 the IPP round
 * loop, 21 the L / R table-lookup MSM of one round (the prover's dominant kernel, nested inside 20).
 * Kind 22: the launches only bpgpu_r1cs_prove_fs and bpgpu_r1cs_prove_fs2_begin / _finish have (their transcript slices, the scalar
 * links between the stages, proof assembly); the stages they chain keep reporting under 16..21.  bpgpu_r1cs_commit_values and
 * bpgpu_mpc_commit_values report their point launches under 16 and the chain launch under 22.
 * Kind 23: the decode launches of bpgpu_r1cs_verify_mixed_wire_* (ragged unpack + point decompression, and the fold of the reject
 * bits: two pairs per check); the ragged transcript replay of those calls reports under 5. */
int bpgpu_profile_enable(bpgpu_ctx *ctx, int on);
int bpgpu_profile_select(bpgpu_ctx *ctx, uint32_t kind_mask);
int bpgpu_profile_read(bpgpu_ctx *ctx, double ms_sum[BPGPU_PROF_KINDS], uint64_t launches[BPGPU_PROF_KINDS]);
/* The same measurements as intervals: bpgpu_profile_epoch records (and waits for) a reference event on ctx's stream and returns
 * its handle (owned by ctx, valid until bpgpu_destroy; NULL on failure); bpgpu_profile_intervals returns every timed launch since
 * the last read -- kind, start and end in milliseconds relative to the epoch of ANY context of the same device -- up to `cap`
 * entries, instead of bpgpu_profile_read's sums.  The union of the intervals of all contexts is the time the GPU was busy:
 * sums of overlapping launches exceed the wall clock, their union cannot. */
void *bpgpu_profile_epoch(bpgpu_ctx *ctx);
int bpgpu_profile_intervals(bpgpu_ctx *ctx, void *epoch, size_t cap, int32_t *kind, double *start_ms, double *end_ms, size_t *count);

/* device memory plumbing */
int bpgpu_malloc(bpgpu_ctx *ctx, size_t bytes, void **dptr);
int bpgpu_free(bpgpu_ctx *ctx, void *dptr);
int bpgpu_upload(bpgpu_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int bpgpu_download(bpgpu_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* the same, enqueued on the context's stream without waiting: the host buffer must stay alive (and should be page-locked:
 * bpgpu_host_alloc) until bpgpu_sync.  A caller streaming batches through `_dev` entry points overlaps the upload of
 * batch i+1 with the kernels of batch i this way (bench.py `h2d_inclusive`). */
int bpgpu_upload_async(bpgpu_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int bpgpu_download_async(bpgpu_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Page-locked host memory for staging.  Operands handed over from such a buffer reach the device by DMA at PCIe
 * speed; pageable buffers go through the runtime's bounce buffers (3-10 GB/s measured).  Optional -- every entry point
 * accepts ordinary host pointers (the Rust side would keep its packed scalar / point staging Vec in one of these).
 * The memory belongs to the process, not to a context.  BPGPU_E_DEVICE without a HIP device, BPGPU_E_OOM. */
int bpgpu_host_alloc(size_t bytes, void **out);
void bpgpu_host_free(void *p);

/* ---- scalar field --------------------------------------------------------------------------
 * Scalar::batch_inverse(&mut [Scalar])   -- src/inner_product_proof.rs:283
 * Scalar::inverse()                      -- src/inner_product_proof.rs:123,181; r1cs/prover.rs:593; r1cs/verifier.rs:468
 * In place.  A zero element -> BPGPU_E_ARG (mpc-stark/ark-ff leave zeros untouched; the reference
 * only passes non-zero challenges). */
int bpgpu_batch_inverse(bpgpu_ctx *ctx, uint8_t *scalars, size_t n);
/* inner_product(a, b)                    -- src/inner_product_proof.rs:463-472 (panics on length
 * mismatch: here the single n makes that unrepresentable) */
int bpgpu_inner_product(bpgpu_ctx *ctx, const uint8_t *a, const uint8_t *b, size_t n, uint8_t out[32]);

/* ---- multi-scalar multiplication ------------------------------------------------------------
 * StarkPoint::msm_iter(scalars, points) / StarkPoint::msm(&[..], &[..])
 *   -- src/r1cs/prover.rs:465,477,485,535,546,555; src/inner_product_proof.rs:90,103,159,166,226-227,353;
 *      src/r1cs/verifier.rs:516.  Accepts identity points, zero scalars, duplicate points, n == 0. */
int bpgpu_msm(bpgpu_ctx *ctx, const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out[64]);
/* nb independent MSMs of n terms each (term-major within an MSM); out = nb points */
int bpgpu_msm_batch(bpgpu_ctx *ctx, size_t nb, size_t n, const uint8_t *scalars, const uint8_t *points,
                    uint8_t *out);
/* bpgpu_msm_batch with device-resident operands and result (boundary encodings in HBM, e.g. from bpgpu_upload):
 * asynchronous on the context's stream; malformed operands raise the context's input flag (bpgpu_input_flag)
 * instead of an error code.  For callers that keep points resident between MSMs. */
int bpgpu_msm_batch_dev(bpgpu_ctx *ctx, size_t nb, size_t n, const void *scalars_dev, const void *points_dev,
                        void *out_dev);
/* Diagnostic, no context and no device needed: the launch route that the bucket method (k_pip.hip: what bpgpu_msm,
 * bpgpu_msm_batch(_dev), bpgpu_msm_ark and bpgpu_msm_shared run from BPGPU_OPT_PIPPENGER_MIN terms on, when the window-parallel
 * launches do not take the call) chooses for nb instances of n terms.  The route depends on (nb, n) alone and never on the data; the
 * library takes its own decisions from the same function, so the tests can assert which kernels a shape reaches.  Results never
 * depend on the route.  out[BPGPU_PIP_PLAN_*]; BPGPU_E_ARG for nb == 0 or n < 2, BPGPU_E_LEN for a shape the 32-bit bucket ids
 * cannot address (the MSM entry points return the same). */
#define BPGPU_PIP_PLAN_C 0            /* window bits: 8..16 */
#define BPGPU_PIP_PLAN_W 1            /* windows: 252 / c + 1 */
#define BPGPU_PIP_PLAN_TWO_LEVEL 2    /* 1: LDS-staged two-level counting sort of the bucket ids, 0: one global atomic per entry */
#define BPGPU_PIP_PLAN_TASK 3         /* entries of a bucket that one lane adds up: 16 or 64 */
#define BPGPU_PIP_PLAN_TASK_SEARCH 4  /* task table: 1 = a lane per task and a binary search, 0 = a lane per bucket and a loop */
#define BPGPU_PIP_PLAN_TASK_SORT 5    /* 1: the tasks are sorted by length before the bucket launch */
#define BPGPU_PIP_PLAN_SCAN 6         /* launches of a scan over the bucket counts: 2 or 3 */
#define BPGPU_PIP_PLAN_COARSE_SCAN 7  /* launches of the scan over the two-level sort's coarse histograms: 2 or 3; 0 without that sort */
#define BPGPU_PIP_PLAN_FINAL_QUAD 8   /* Horner tail: 1 = a quad per instance, 0 = a wave per instance */
#define BPGPU_PIP_PLAN_CHUNKS 9       /* blocks a window's running sum is cut into: 1..64 */
#define BPGPU_PIP_PLAN_FIELDS 10
int bpgpu_pippenger_plan(size_t nb, size_t n, int32_t out[BPGPU_PIP_PLAN_FIELDS]);
/* sum of n points, no scalars (StarkPoint + StarkPoint): the local reduction of the <= 8 partial results that the GPUs of
 * a node all-gather after a term-range-sharded MSM or a combined batch check -- one launch instead of an
 * MSM with unit scalars (whose 252-doubling chain costs ~1 ms however few the terms). */
int bpgpu_points_sum(bpgpu_ctx *ctx, const uint8_t *points, size_t n, uint8_t out[64]);
/* ---- arkworks in-memory forms: zero-copy hand-over from the Rust host --------------------------------
 * mpc-stark's Scalar is ark_ff::Fp256<MontBackend<_, 4>>: four little-endian u64 limbs holding x * 2^256 mod n (32 bytes as
 * they lie in memory); its StarkPoint is ark_ec::short_weierstrass::Projective: Jacobian (X : Y : Z), the point is
 * (X / Z^2, Y / Z^3), each coordinate four u64 limbs holding c * 2^256 mod p (96 bytes), identity Z = 0.  These entry points take
 * and return exactly those bytes: no de-Montgomery / serialisation / inversion on the host (one Montgomery multiplication per
 * element on the device instead).  Non-canonical limbs (>= modulus) and points off the curve -> BPGPU_E_ARG.
 *   bpgpu_msm_ark            StarkPoint::msm / msm_iter with operands and result in arkworks form
 *                            -- verifier.rs:516-547, prover.rs:465-564, inner_product_proof.rs:90-172
 *   bpgpu_scalars_from_ark / _to_ark, bpgpu_points_from_ark / _to_ark: convert whole vectors to / from the boundary encodings
 *                            (32-byte LE canonical scalars, 64-byte affine x || y) that every other entry point takes. */
int bpgpu_msm_ark(bpgpu_ctx *ctx, const uint8_t *scalars_mont, const uint8_t *points_jac_mont, size_t n,
                  uint8_t out_jac_mont[96]);
int bpgpu_scalars_from_ark(bpgpu_ctx *ctx, const uint8_t *scalars_mont, size_t n, uint8_t *scalars_le);
int bpgpu_scalars_to_ark(bpgpu_ctx *ctx, const uint8_t *scalars_le, size_t n, uint8_t *scalars_mont);
int bpgpu_points_from_ark(bpgpu_ctx *ctx, const uint8_t *points_jac_mont, size_t n, uint8_t *points_xy);
int bpgpu_points_to_ark(bpgpu_ctx *ctx, const uint8_t *points_xy, size_t n, uint8_t *points_jac_mont);
/* nsets MSMs over ONE point vector: out[s] = sum_i scalars[s*n + i] * points[i].  This is the local work of
 * StarkPoint::msm_authenticated_iter in the two-party prover -- one MSM each over the secret shares, the MACs and
 * the public modifiers of the same authenticated scalars against the same points (r1cs_mpc/mpc_prover.rs:621-657,
 * 717-750; r1cs_mpc/mpc_inner_product.rs:104-126,172-186): the points are validated and converted
 * once.  scalars: nsets x n x 32 B; points: n x 64 B; out: nsets x 64 B. */
int bpgpu_msm_shared(bpgpu_ctx *ctx, size_t nsets, size_t n, const uint8_t *scalars, const uint8_t *points,
                     uint8_t *out);

/* ---- resident generators ---------------------------------------------------------------------
 * BulletproofGens::share(0).G(n) / .H(n) and PedersenGens{B, B_blinding}
 *   -- src/generators.rs:32-37,158-167,310-320.  Uploads the points once and precomputes signed
 * fixed-window tables (window_bits in {4, 8, 10, 12, 14, 16, 20}; table bytes = (2*cap+2) * (252/c+1) * 2^(c-1) * 64). */
int bpgpu_gens_create(bpgpu_ctx *ctx, const uint8_t *G, const uint8_t *H, size_t gens_capacity,
                      const uint8_t B[64], const uint8_t B_blinding[64], int window_bits,
                      bpgpu_gens **out);
void bpgpu_gens_destroy(bpgpu_ctx *ctx, bpgpu_gens *g);
size_t bpgpu_gens_capacity(const bpgpu_gens *g);
/* sum_i s_i * X_i over the resident set, nb independent scalar vectors.  Layout of one vector:
 * [B, B_blinding, G_0..G_{n-1}, H_0..H_{n-1}] (2 + 2n scalars), n <= capacity.
 *   -- the generator part of prover.rs:465-494 and verifier.rs:525-530,541-544 */
int bpgpu_msm_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *scalars,
                   uint8_t *out);
/* the same with the scalars as they lie in the reference's memory (ark-ff Montgomery limbs, x * 2^256 mod n, 4 x u64 little
 * endian; see the arkworks section below): converted on the device, no de-Montgomery per scalar on the host.  The 256
 * lock-step provers of BASELINE configs[2] hand over 1.3 M witness and blinding scalars per batch this way. */
int bpgpu_msm_gens_ark(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *scalars_ark,
                       uint8_t *out);

/* ---- inner-product argument ------------------------------------------------------------------
 * InnerProductProof::fold_witness  -- src/inner_product_proof.rs:202-248
 * Inputs hold [L half || R half] (2n entries each); outputs n entries:
 *   a' = a_L u + u^-1 a_R ; b' = b_L u^-1 + u b_R ; G' = u^-1 G_L + u G_R ; H' = u H_L + u^-1 H_R */
int bpgpu_fold_witness(bpgpu_ctx *ctx, size_t n, const uint8_t u[32], const uint8_t u_inv[32],
                       const uint8_t *a, const uint8_t *b, const uint8_t *G, const uint8_t *H,
                       uint8_t *a_out, uint8_t *b_out, uint8_t *G_out, uint8_t *H_out);
/* arithmetic half of InnerProductProof::verification_scalars -- src/inner_product_proof.rs:280-309
 * challenges u_1..u_k (creation order) -> u_sq[k], u_inv_sq[k], s[n], n == 2^k else BPGPU_E_LEN
 * (the transcript replay of :271-278 stays on the host). */
int bpgpu_verification_scalars(bpgpu_ctx *ctx, const uint8_t *challenges, size_t k, size_t n,
                               uint8_t *u_sq, uint8_t *u_inv_sq, uint8_t *s);
/* InnerProductProof::verify -- src/inner_product_proof.rs:317-372 -- for nb proofs of one length n = 2^k in one call:
 *   expect_P = a b Q + sum_i a s_i Gf_i G_i + sum_i b s_{n-1-i} Hf_i H_i - sum_j u_j^2 L_j - sum_j u_j^-2 R_j ;  ok[p] = 1 iff expect_P == P
 * (the vector s of :280-309 stays on the device and is never stored).
 * Q, P: nb x 64 B; G_factors, H_factors: nb x n x 32 B; G, H: n x 64 B shared by all proofs (shared_gens = 1) or nb x n x 64 B;
 * L, R: nb x k x 64 B (proof-major); ab: nb x 2 x 32 B (a, b); challenges: nb x k x 32 B, u_1..u_k in creation order, from the
 * host's transcript replay (:269-278).  ok: nb int32.  expect_P (optional): nb x 64 B, for accepted and rejected proofs alike.
 * G_factors and H_factors hold exactly n entries per proof: the reference's .take(G.len()) over a longer iterator is not
 * reproduced.  k >= 32 or n != 2^k: BPGPU_E_LEN (:259-267); a null operand: BPGPU_E_ARG (L, R, challenges may be null when k = 0);
 * a size one of the MSM routes cannot address: BPGPU_E_LEN, as bpgpu_msm_batch; nb == 0: BPGPU_OK.  A non-canonical scalar or an
 * off-curve / non-canonical point is BPGPU_E_ARG.  A wrong proof is never an error: ok[p] = 0; so is one with a zero challenge
 * (the reference's batch inversion has no inverse to give). */
int bpgpu_ipp_verify_batch(bpgpu_ctx *ctx, size_t nb, size_t n, size_t k, const uint8_t *Q, const uint8_t *G_factors,
                           const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int shared_gens, const uint8_t *P,
                           const uint8_t *L, const uint8_t *R, const uint8_t *ab, const uint8_t *challenges, int32_t *ok,
                           uint8_t *expect_P);
/* The same on device pointers (bpgpu_malloc), asynchronous on the context's stream: results are valid after bpgpu_sync, and a
 * malformed operand raises bpgpu_input_flag instead of an error code (the verdicts of such a call mean nothing). */
int bpgpu_ipp_verify_batch_dev(bpgpu_ctx *ctx, size_t nb, size_t n, size_t k, const void *Q, const void *G_factors,
                               const void *H_factors, const void *G, const void *H, int shared_gens, const void *P, const void *L,
                               const void *R, const void *ab, const void *challenges, void *ok, void *expect_P);
/* Over RESIDENT generators: G, H = the first n of `g`, Q = w * B with B = g's Pedersen base (w: nb x 32 B), as
 * bpgpu_ipp_begin_gens; the generator half is a table walk.  n above g's capacity: BPGPU_E_GENS. */
int bpgpu_ipp_verify_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, const uint8_t *w,
                          const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *L, const uint8_t *R,
                          const uint8_t *ab, const uint8_t *challenges, int32_t *ok, uint8_t *expect_P);
/* With the transcript replay on the DEVICE: per proof k x (validate_and_append_point "L", "R"; challenge_scalar "u") from
 * states_in, the nb 32-byte hash-chain states after innerproduct_domain_sep (the convention of bpgpu_ipp_run_fs); states_out
 * (optional): the states afterwards.  An identity L or R rejects its proof (transcript.rs validate_and_append_point): ok[p] = 0,
 * not an error.  g == NULL: Q_or_w = Q and G, H, shared_gens as in bpgpu_ipp_verify_batch; otherwise resident generators and
 * Q_or_w = w (G, H ignored).  The hash chain is the build's stand-in for merlin's. */
int bpgpu_ipp_verify_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, size_t k, const uint8_t *Q_or_w,
                        const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int shared_gens,
                        const uint8_t *P, const uint8_t *L, const uint8_t *R, const uint8_t *ab, const uint8_t *states_in,
                        int32_t *ok, uint8_t *states_out);

/* InnerProductProof::create -- src/inner_product_proof.rs:49-193 -- split at the Fiat-Shamir transcript
 * (which stays on the host) for nb independent proofs advancing in lock-step; all state stays in HBM
 * between rounds.  n must be a power of two (reference asserts, :70).  G/H: n points shared by all
 * proofs (shared_gens = 1) or nb x n.  Protocol per round while bpgpu_ipp_len() > 1:
 *   bpgpu_ipp_round -> L[nb], R[nb]   (c_L, c_R :87-88,156-157 and the two MSMs :90-114,159-172;
 *                                       the first round folds G_factors/H_factors into the scalars)
 *   host: append L, R; u = challenge; u_inv = u.inverse()              (:119-123,177-181)
 *   bpgpu_ipp_fold(u[nb], u_inv[nb])  (first round also scales the generators, :125-134; then
 *                                       fold_witness :135-146,183-184)
 * then bpgpu_ipp_finish -> a[nb], b[nb] (:187-192). */
typedef struct bpgpu_ipp bpgpu_ipp;
int bpgpu_ipp_begin(bpgpu_ctx *ctx, size_t nb, size_t n, const uint8_t *Q, const uint8_t *G_factors,
                    const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int shared_gens,
                    const uint8_t *a, const uint8_t *b, bpgpu_ipp **out);
/* The same session over RESIDENT generators (G, H = the first n of `g`, Q = w * B with B = g's Pedersen base:
 * exactly what r1cs/prover.rs:687-708 passes).  No generator is ever folded: round j's L, R are fixed-base
 * MSMs over the original generators with the accumulated challenge products folded into the scalars, so a
 * round costs table lookups instead of two 252-doubling chains.  Same outputs as bpgpu_ipp_begin.
 * w: nb x 32 B. */
int bpgpu_ipp_begin_gens(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t n, const uint8_t *w,
                         const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *a, const uint8_t *b,
                         bpgpu_ipp **out);
/* All remaining rounds of a session with the transcript on the DEVICE (SURVEY 8f N1 applied to the prover): per round
 * L, R, transcript.append_point("L" / "R"), challenge_scalar("u") (inner_product_proof.rs:119-123, 177-181), u^-1 and
 * the fold, back to back on the stream -- no host round trip per round.  states_in: the provers' 32-byte hash-chain
 * states after innerproduct_domain_sep (:72); L_out / R_out: nb x k x 64 B (proof-major); a_out, b_out: nb x 32 B;
 * states_out (optional): the chain states afterwards.  The hash chain is the build's stand-in for merlin's. */
int bpgpu_ipp_run_fs(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *states_in, uint8_t *L_out, uint8_t *R_out,
                     uint8_t *a_out, uint8_t *b_out, uint8_t *states_out);
void bpgpu_ipp_destroy(bpgpu_ctx *ctx, bpgpu_ipp *s);
size_t bpgpu_ipp_len(const bpgpu_ipp *s);
int bpgpu_ipp_round(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *L, uint8_t *R);
int bpgpu_ipp_fold(bpgpu_ctx *ctx, bpgpu_ipp *s, const uint8_t *u, const uint8_t *u_inv);
int bpgpu_ipp_finish(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *a_out, uint8_t *b_out);
/* Resident-generator sessions only, after the last fold (bpgpu_ipp_len == 1): the folded generators as points,
 * G' = sum_i cG[i] G_i and H' = sum_i cH[i] H_i (nb x 64 B each) -- the pair the final (a, b) refers to.  A rank of a
 * vector-sharded IPP (one proof's a, b, G, H dealt cyclically over the GPUs of a node: SURVEY 8e.2,
 * mpc_bulletproof_amd/sharding.py sharded_ipp_create) hands (a, b, G', H') to the last log2(ranks) rounds. */
int bpgpu_ipp_folded_gens(bpgpu_ctx *ctx, bpgpu_ipp *s, uint8_t *G_out, uint8_t *H_out);

/* ---- R1CS ------------------------------------------------------------------------------------
 * Constraint rows as the reference holds them (Vec<LinearCombination>, r1cs/prover.rs:31,
 * r1cs/verifier.rs:38): CSR with row_ptr[q+1]; per term kind (0 MultiplierLeft, 1 MultiplierRight,
 * 2 MultiplierOutput, 3 Committed, 4 One -- linear_combination.rs:15-28), index, coefficient. */
int bpgpu_circuit_create(bpgpu_ctx *ctx, size_t q, const uint32_t *row_ptr, const uint32_t *kind,
                         const uint32_t *idx, const uint8_t *coeff, size_t n_multipliers,
                         size_t m_commitments, bpgpu_circuit **out);
void bpgpu_circuit_destroy(bpgpu_ctx *ctx, bpgpu_circuit *c);
/* Prover/Verifier::flattened_constraints(z) -- r1cs/prover.rs:342-379, r1cs/verifier.rs:323-362.
 * nb challenges z (one per proof) -> wL,wR,wO (nb x n), wV (nb x m), wc (nb) ; wc may be NULL (prover). */
int bpgpu_flatten_constraints(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *z,
                              uint8_t *wL, uint8_t *wR, uint8_t *wO, uint8_t *wV, uint8_t *wc);

/* bpgpu_circuit_create with the coefficients as they lie in the reference's memory (ark-ff Montgomery limbs, x * 2^256 mod n):
 * converted on the device.  The 2^14-shuffle's ~200 000 coefficients cost the host 8 ms of de-Montgomery per upload otherwise. */
int bpgpu_circuit_create_ark(bpgpu_ctx *ctx, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                             const uint8_t *coeff_ark, size_t n_multipliers, size_t m_commitments, bpgpu_circuit **out);
/* Circuits with RANDOMIZED (second-phase) constraints whose coefficients are affine in the gadget's challenge
 * (RandomizableConstraintSystem::specify_randomized_constraints + cs.challenge_scalar(label) -- r1cs/verifier.rs:366-385,
 * r1cs/prover.rs:383-402; the shuffle gadget (x_i - z), tests/r1cs.rs:23-62): coefficient of a term = c0 + sum_j chi_j * c_j.
 * The CSR has (1 + nchi) * q rows: rows [0, q) hold the constant parts c0, rows [j q, (j + 1) q) the chi_j parts (row r of block j
 * belongs to constraint r).  One such circuit serves every proof of the gadget, whatever challenge its transcript produced.
 * Use it with bpgpu_r1cs_verify_batch_param (gadget challenges from the host) or bpgpu_r1cs_verify_batch_fs2 (transcript on the
 * device); the other entry points reject it (BPGPU_E_ARG).  nchi <= 8.  The device transcript draws one challenge under the label
 * an entry point is given, or all nchi under the circuit's own labels (bpgpu_circuit_set_gadget_labels). */
int bpgpu_circuit_create_param(bpgpu_ctx *ctx, size_t q, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                               const uint32_t *idx, const uint8_t *coeff, size_t n_multipliers, size_t m_commitments,
                               bpgpu_circuit **out);
/* The labels of a parametric circuit's gadget challenges: nchi x 32 bytes, each zero-padded as gadget_label.  Label j is the label of
 * the j-th challenge_scalar call of the randomized phase, in draw order (the closures run one after the other, r1cs/prover.rs:383-408,
 * r1cs/verifier.rs:366-385) -- the challenge whose parts are block j + 1 of the circuit's rows.  The handle keeps a copy (host memory);
 * a later call replaces it.  Not to be called while another call uses the handle.  BPGPU_E_ARG: a null pointer, a numeric circuit.
 * Every entry point with the transcript on the device -- bpgpu_r1cs_prove_fs2_begin / _finish, bpgpu_r1cs_prove_fs2,
 * bpgpu_r1cs_prove_values, bpgpu_r1cs_verify_batch_fs2, bpgpu_r1cs_verify_batch_wire2, bpgpu_r1cs_verify_mixed_wire_* -- then takes the
 * circuit with gadget_label == NULL (a label beside attached ones: BPGPU_E_ARG), for any 1 <= nchi <= 8: TS step j hashes under
 * label j, and every gadget_challenges(_out) array is nb x nchi x 32, prover-major.  A circuit with nothing attached behaves as
 * described at each entry point: one challenge, under the label given.  Timings of circuits with nchi > 1: UNMEASURED. */
int bpgpu_circuit_set_gadget_labels(bpgpu_ctx *ctx, bpgpu_circuit *c, const uint8_t *labels);
/* Prover::prove arithmetic between the y,z and the u,x challenges -- r1cs/prover.rs:587-619:
 * flattened_constraints(z), exp_y / exp_y_inv, the l(x)/r(x) coefficient vectors and
 * t_1..t_6 = VecPoly3::special_inner_product (util.rs:152-170), for nb provers of ONE circuit.
 * Inputs proof-major: y, y_inv, z (nb); a_L, a_R, a_O, s_L, s_R (nb x n, n = multipliers).
 * Outputs: t_coeffs nb x 6 (t1 t2 t3 t4 t5 t6), wV nb x m (for t_2_blinding, prover.rs:644-648).
 * The coefficient vectors stay in HBM in *out for bpgpu_r1cs_prover_eval -- prover.rs:659-672:
 * l_vec, r_vec (nb x padded_n) = l(x), r(x) with the zero / -y^i padding. */
typedef struct bpgpu_prover bpgpu_prover;
int bpgpu_r1cs_prover_polys(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *y,
                            const uint8_t *y_inv, const uint8_t *z, const uint8_t *a_L, const uint8_t *a_R,
                            const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, uint8_t *t_coeffs,
                            uint8_t *wV, bpgpu_prover **out);
/* the same with every INPUT scalar (y, y_inv, z, a_L, a_R, a_O, s_L, s_R) in ark-ff Montgomery form; outputs as above */
int bpgpu_r1cs_prover_polys_ark(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *y,
                                const uint8_t *y_inv, const uint8_t *z, const uint8_t *a_L, const uint8_t *a_R,
                                const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, uint8_t *t_coeffs,
                                uint8_t *wV, bpgpu_prover **out);
int bpgpu_r1cs_prover_eval(bpgpu_ctx *ctx, bpgpu_prover *s, size_t padded_n, const uint8_t *x,
                           uint8_t *l_vec, uint8_t *r_vec);
/* prover.rs:659-708 in one call with everything staying in HBM: evaluates l(x), r(x) (with the padding), forms
 * G_factors = [1; n1] ++ [u; padded_n - n1] and H_factors = y^-i * G_factors (prover.rs:689-697) and opens the
 * resident-generator IPP session (bpgpu_ipp_begin_gens) on them with Q = w * B.  x, u, y_inv, w: nb x 32 B.
 * Continue with bpgpu_ipp_round / fold / finish. */
int bpgpu_r1cs_prover_ipp_begin(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_gens *g, size_t padded_n, size_t n1,
                                const uint8_t *x, const uint8_t *u, const uint8_t *y_inv, const uint8_t *w,
                                bpgpu_ipp **out);
void bpgpu_prover_destroy(bpgpu_ctx *ctx, bpgpu_prover *s);
/* Resident-witness prover sessions: the same Prover::prove arithmetic with the witness crossing the bus ONCE and, optionally, the
 * blinding vectors never crossing it at all (256 provers x 1024 multipliers: 25 MB up instead of 92 MB, no 525 000 host-side
 * scalar draws).  All scalars in ark-ff Montgomery form unless stated.
 *
 * bpgpu_r1cs_prover_commit -- r1cs/prover.rs:457-494 (first call: *session == NULL, phase-1 multipliers) and :519-565 (second call
 *   on the same session: the n_new multipliers the randomized constraints added; skip it when there are none -- the reference sets
 *   A_I2 = A_O2 = S2 = identity, :566-576).  a_L, a_R, a_O: nb x n_new.  Blinding vectors s_L, s_R (:461-462, :526-527): either
 *   explicit (nb x n_new each; vector_keys NULL) or drawn on the device from vector_keys (nb x 32 raw bytes the caller takes from
 *   its RNG where the reference draws the vectors; s_L = s_R = NULL): "BlindVec v1",
 *     block(key, v, j) = first 128 bytes of Keccak-f[1600] over the padded 48-byte message key || u64le(v) || u64le(j)   (v = 0: s_L, 1: s_R)
 *     s_v[i] = int_LE(block(key, v, i / 2)[64 (i mod 2) .. +64]) mod n
 *   (the CPU oracle restates the stream, so such proofs replay under a test RNG).  blindings: nb x 3 (i_blinding, o_blinding,
 *   s_blinding).  commitments out: nb x 3 x 64 B (A_I, A_O, S).  BPGPU_E_GENS when the multipliers exceed the generators.
 * bpgpu_r1cs_prover_session_polys -- :587-619 on the session's planes: y^-1 (:593, on the device), flattened constraints, l / r
 *   coefficient vectors, t_1..t_6.  y, z: nb x 32 B canonical LE (fresh transcript challenges); outputs as bpgpu_r1cs_prover_polys.
 *   Continue with bpgpu_r1cs_prover_ipp_begin, whose y_inv may then be NULL (the session's own). */
int bpgpu_r1cs_prover_commit(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover **session, size_t nb, size_t n_new,
                             const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                             const uint8_t *vector_keys, const uint8_t *blindings, uint8_t *commitments);
int bpgpu_r1cs_prover_session_polys(bpgpu_ctx *ctx, bpgpu_prover *s, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                    uint8_t *t_coeffs, uint8_t *wV);
/* The same for a circuit of bpgpu_circuit_create_param (second-phase constraints affine in the gadget challenges, prover.rs:383-402):
 * gadget_challenges = nb x nchi x 32 bytes, the values the provers' transcripts produced.  The rows of such a circuit cross the ABI
 * once per circuit shape; a prover of the 2^14-shuffle no longer builds and uploads 65 533 constraint rows per proof. */
int bpgpu_r1cs_prover_session_polys_param(bpgpu_ctx *ctx, bpgpu_prover *session, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                          const uint8_t *gadget_challenges, uint8_t *t_coeffs, uint8_t *wV);
/* Prover::prove (r1cs/prover.rs:412-727) in ONE call, transcript included, for nb provers of one circuit WITHOUT randomized constraints
 * (bpgpu_circuit_create / _ark): the phase commitments, y and z, the polynomial build, the T commitments, u and x, t(x) and the
 * blindings, w, the IPP session and its k rounds run back to back on the context's stream; the Fiat-Shamir hash chain is advanced on
 * the device between them.  It replaces the five staged calls (bpgpu_r1cs_prover_commit, _session_polys, bpgpu_msm_gens,
 * bpgpu_r1cs_prover_ipp_begin, bpgpu_ipp_run_fs) and the host hashing, waits and copies between them.  A parametric circuit
 * (bpgpu_circuit_create_param) is refused with BPGPU_E_ARG: the phase-2 witness of a two-phase prover depends on the gadget's
 * challenge.  A host round trip is inherent only to a gadget that no bpgpu_witness gate program describes: such provers take
 * bpgpu_r1cs_prove_fs2_begin / _finish (two calls around a gadget that the host evaluates), every other two-phase prover
 * bpgpu_r1cs_prove_fs2 (one call: the gates evaluated on the device).
 * With n = the circuit's multipliers, m its commitments, padded_n = next_pow2(n), k = lg padded_n:
 *   states_in      nb x 32        the chain state on entry to Prover::prove (prover.rs:412): after Prover::new and every commit(),
 *                                 i.e. the V's are already absorbed by the host
 *   a_L, a_R, a_O  nb x n         ark-ff Montgomery form
 *   s_L, s_R       nb x n         explicit blinding vectors, or both NULL with
 *   vector_keys    nb x 32        "BlindVec v1" keys, as bpgpu_r1cs_prover_commit (exactly one of the two sources)
 *   v_blinding     nb x m         ark form (prover.rs:644-648); may be NULL when m == 0
 *   blindings      nb x 8         ark form: i_blinding o_blinding s_blinding tb1 tb3 tb4 tb5 tb6, in the order the reference draws
 *                                 them (:457-459, :621-625); the transcript-bound RNG of :435-445 is the caller's
 *   proof_points   nb x (11 + 2k) x 64   A_I1 A_O1 S1 A_I2 A_O2 S2 T_1 T_3 T_4 T_5 T_6 L_0..L_{k-1} R_0..R_{k-1}; A_I2, A_O2, S2 are
 *                                 the identity (64 zero bytes) and are absorbed as such
 *   proof_scalars  nb x 5 x 32    canonical LE: t_x t_x_blinding e_blinding a b (layout of bpgpu_r1cs_verify_batch)
 *   wire           (optional) nb x proof_len, proof_len = 1 + 11 * 32 + (2k + 2) * 32: R1CSProof::to_bytes (proof.rs:82-109), version
 *                                 byte 0 (which omits the three identity points)
 *   challenges_out (optional) nb x (5 + k) x 32: y z u x w u_1..u_k;   states_out (optional) nb x 32: the chain states afterwards
 * Refusals, before anything is launched: BPGPU_E_ARG for a null required pointer, for both or neither of explicit s_L / s_R and
 * vector_keys, for a parametric circuit and for a context after bpgpu_set_shard(world > 1); BPGPU_E_LEN for n == 0 (the staged calls
 * remain for such circuits); BPGPU_E_GENS for padded_n above the generators' capacity; nb == 0: BPGPU_OK.  A non-canonical ark limb
 * gives BPGPU_E_ARG in the host form and raises bpgpu_input_flag in the `_dev` form (every operand and result a device pointer;
 * asynchronous on the context's stream).  A failed call leaves no session or pool memory behind.  The hash chain is the build's
 * stand-in for merlin's. */
int bpgpu_r1cs_prove_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const uint8_t *states_in,
                        const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                        const uint8_t *vector_keys, const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points,
                        uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out);
int bpgpu_r1cs_prove_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, const void *states_in,
                            const void *a_L, const void *a_R, const void *a_O, const void *s_L, const void *s_R,
                            const void *vector_keys, const void *v_blinding, const void *blindings, void *proof_points,
                            void *proof_scalars, void *wire, void *challenges_out, void *states_out);
/* Prover::commit (r1cs/prover.rs:319-329) for the m committed values of each of nb provers -- the step BEFORE the calls above and
 * below: V = v B + v_blinding B_blinding (PedersenGens::commit, generators.rs:41-43) over g's resident Pedersen pair (table generators
 * 0 and 1; the pair may be equal, as in the reference's default PedersenGens) and, optionally, the chain from Prover::new to the last
 * commit.  A host that holds (init_state, v, v_blinding, witness, blindings) on the device enqueues bpgpu_r1cs_commit_values_dev ->
 * bpgpu_r1cs_constraints_satisfied_dev -> bpgpu_r1cs_prove_fs_dev without a wait or a copy, and gets back what the wire verifiers take.
 *   v, v_blinding  nb x m         ark-ff Montgomery form: the buffers bpgpu_r1cs_constraints_satisfied takes as v and
 *                                 bpgpu_r1cs_prove_fs as v_blinding (one set of device buffers serves all three calls); may be NULL
 *                                 when nb m == 0
 *   states_in      (optional) nb x 32   the chain state when the host would call Prover::new: the value the _fs / _wire verifiers take
 *                                 as init_states
 *   V              (optional) nb x m x 64   boundary form
 *   V_compressed   (optional) nb x m x 32   the form bpgpu_points_compress writes and bpgpu_r1cs_verify_batch_wire reads as commitments
 *   states_out     (optional) nb x 32   the chain after r1cs_domain_sep (prover.rs:286) and m x append_point("V", V_j) in order: exactly
 *                                 the states_in of bpgpu_r1cs_prove_fs / bpgpu_r1cs_prove_fs2_begin
 * states_in and states_out go together: both, or neither (no transcript).  At least one of V, V_compressed, states_out must be given.
 * A prover does not validate: an identity commitment (v = v_blinding = 0, or v + v_blinding = 0 mod n over equal bases) is written as
 * 64 zero bytes, compressed as 00..00 40 (31 zero bytes, then 0x40) and absorbed as 64 zero bytes.  m == 0 is legal: no points, and
 * states_out is the state after the separator.
 * Refusals, before anything is launched: BPGPU_E_ARG for a null context or gens, for a null v or v_blinding while nb m > 0, for
 * exactly one of states_in / states_out, for no output at all and for a context after bpgpu_set_shard(world > 1); BPGPU_E_LEN for
 * nb m above 2^30 (the launches index commitments and rows of two scalars with room to spare below that; the two-party call counts
 * its three planes: 3 nb m); nb == 0: BPGPU_OK, no output touched.  A non-canonical ark limb gives BPGPU_E_ARG in the host form and
 * raises bpgpu_input_flag in the `_dev` form (every operand and result a device pointer; asynchronous on the context's stream).  A
 * failed call leaves no pool memory behind.  Profiling: the point launches report under kind 16, the chain launch under kind 22.
 * The chain of ONE prover is serial: a lane absorbs its m points one after the other.  For m in the tens of thousands (the
 * 2^14-shuffle's 32 768 commitments) the host's hashing is faster than one lane -- DESIGN.md gives 9-13 ms for the host; the device
 * figure is not measured -- so such a caller passes states_in = states_out = NULL, takes the points from the call and absorbs them on
 * the host. */
int bpgpu_r1cs_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const uint8_t *v, const uint8_t *v_blinding,
                             const uint8_t *states_in, uint8_t *V, uint8_t *V_compressed, uint8_t *states_out);
int bpgpu_r1cs_commit_values_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const void *v, const void *v_blinding,
                                 const void *states_in, void *V, void *V_compressed, void *states_out);
/* Prover::prove for nb provers of ONE two-phase circuit (bpgpu_circuit_create_param with nchi == 1) in TWO calls around the gadget, for a
 * host that evaluates its gadget on the challenge itself (a gadget that a bpgpu_witness gate program describes needs no round trip:
 * bpgpu_r1cs_prove_fs2 below issues both chains in one call).  The Fiat-Shamir hash
 * chain runs on the device in both calls; they replace bpgpu_r1cs_prover_commit (twice), _session_polys_param, bpgpu_msm_gens,
 * bpgpu_r1cs_prover_ipp_begin, bpgpu_ipp_run_fs and the host hashing between them.  With n = the circuit's multipliers, n1 those of
 * phase 1, n2 = n - n1 >= 1, m its commitments, padded_n = next_pow2(n), k = lg padded_n:
 * _begin (prover.rs:420-501): append_u64("m"), the phase-1 commitments (n1 == 0 commits the blindings alone), A_I1 A_O1 S1 absorbed,
 * the 2-phase separator, challenge_scalar(gadget_label) -- the label zero-padded to 32 bytes as in bpgpu_r1cs_verify_batch_fs2; NULL
 * for a circuit with attached labels (bpgpu_circuit_set_gadget_labels), which draws its nchi challenges, each under its own.
 *   states_in      nb x 32        the chain state on entry to Prover::prove, as bpgpu_r1cs_prove_fs
 *   a_L, a_R, a_O  nb x n1        ark form; s_L, s_R nb x n1 or vector_keys nb x 32: exactly one source when n1 > 0; all may be NULL
 *                                 when n1 == 0
 *   blindings      nb x 3         ark form: i_blinding1 o_blinding1 s_blinding1 (:457-459)
 *   session        in: *session == NULL; out: the open session.  It keeps on the device the chain state, the gadget challenges (nb x nchi x 32 B), the
 *                                 phase-1 blinding factors and commitments and the witness planes
 *   commitments    (optional) nb x 3 x 64: A_I1 A_O1 S1;   gadget_challenges_out (optional) nb x nchi x 32 canonical LE;
 *   states_out     (optional) nb x 32: the chain after the gadget challenge
 * _finish (:515-727): the phase-2 commitments over G[n1..n), H[n1..n), A_I2 A_O2 S2 absorbed, y, z, the polynomial build with the
 * parametric weights taken from the session's own gadget challenge, the T commitments, u, x, tb2, t_x, t_x_blinding,
 * e_blinding = x((i1 + u i2) + x((o1 + u o2) + x(s1 + u s2))), w, the IPP session with G_factors = [1; n1] ++ [u; n2 + pad], its k
 * rounds, proof assembly -- without a host wait in between.
 *   a_L, a_R, a_O  nb x n2        ark form; s_L, s_R nb x n2 or vector_keys nb x 32 (exactly one of the two sources)
 *   v_blinding     nb x m         ark form; may be NULL when m == 0
 *   blindings      nb x 8         ark form: i_blinding2 o_blinding2 s_blinding2 tb1 tb3 tb4 tb5 tb6 (draw order of :519-523, :621-625)
 *   proof_points   nb x (11 + 2k) x 64   A_I1 A_O1 S1 A_I2 A_O2 S2 T_1 T_3 T_4 T_5 T_6 L_0..L_{k-1} R_0..R_{k-1}, all real points
 *   proof_scalars  nb x 5 x 32    canonical LE: t_x t_x_blinding e_blinding a b
 *   wire           (optional) nb x proof_len, proof_len = 1 + 14 * 32 + (2k + 2) * 32: R1CSProof::to_bytes with version byte 1 and all
 *                                 14 points
 *   challenges_out (optional) nb x (5 + k) x 32: y z u x w u_1..u_k;   states_out (optional) nb x 32
 * Sessions: _finish consumes the session and sets *session = NULL once anything has been launched, whatever it then returns; a
 * refusal on shapes or arguments leaves it open; bpgpu_prover_destroy frees an abandoned one.  The staged calls (_commit,
 * _session_polys(_param), _eval, _ipp_begin) refuse a session opened by _begin with BPGPU_E_ARG; _finish refuses a session that _begin
 * did not open, and a circuit handle other than the one _begin was given.
 * Refusals, before anything is launched: BPGPU_E_ARG for a null required pointer, for *session != NULL on _begin, for a numeric
 * circuit or nchi != 1, for both or neither source of a phase's blinding vectors when that phase has multipliers, and for a context
 * after bpgpu_set_shard(world > 1); BPGPU_E_LEN for n1 >= n (no second-phase commitments: the staged calls remain for that case);
 * BPGPU_E_GENS for padded_n above the generators' capacity; nb == 0: BPGPU_OK with *session left NULL.  A non-canonical ark limb gives
 * BPGPU_E_ARG in the host forms and raises bpgpu_input_flag in the `_dev` forms (every operand and result a device pointer;
 * asynchronous on the context's stream: _finish_dev may be enqueued right after _begin_dev, without a synchronise, by a host whose
 * phase-2 witness is already resident).  A failed call leaves no pool memory behind. */
int bpgpu_r1cs_prove_fs2_begin(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const uint8_t *states_in,
                               const uint8_t gadget_label[32], const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                               const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *blindings,
                               bpgpu_prover **session, uint8_t *commitments, uint8_t *gadget_challenges_out, uint8_t *states_out);
int bpgpu_r1cs_prove_fs2_begin_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, const void *states_in,
                                   const uint8_t gadget_label[32], const void *a_L, const void *a_R, const void *a_O, const void *s_L,
                                   const void *s_R, const void *vector_keys, const void *blindings, bpgpu_prover **session,
                                   void *commitments, void *gadget_challenges_out, void *states_out);
int bpgpu_r1cs_prove_fs2_finish(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const uint8_t *a_L,
                                const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys,
                                const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points, uint8_t *proof_scalars,
                                uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out);
int bpgpu_r1cs_prove_fs2_finish_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, bpgpu_prover **session, const void *a_L,
                                    const void *a_R, const void *a_O, const void *s_L, const void *s_R, const void *vector_keys,
                                    const void *v_blinding, const void *blindings, void *proof_points, void *proof_scalars, void *wire,
                                    void *challenges_out, void *states_out);
/* Prover::constraints_satisfied (prover.rs:405-409) for nb provers of ONE circuit, where their witnesses lie: the provers above never
 * read the rows' constants and take a_O from the caller, so a wrong witness yields a well-formed proof that fails only at the verifier;
 * this call says so before the proof is paid for.  Circuits of bpgpu_circuit_create / _ark and of bpgpu_circuit_create_param (any
 * nchi <= 8).  With n = ALL the circuit's multipliers (both phases), m its commitments, q its constraints:
 *   a_L, a_R, a_O  nb x n         ark-ff Montgomery form, as bpgpu_r1cs_prove_fs takes them (one set of device buffers serves the
 *                                 check and the proof); may be NULL when n == 0
 *   v              nb x m         the committed VALUES (not the commitments), ark form; may be NULL when m == 0
 *   gadget_challenges  nb x nchi x 32  canonical LE for a parametric circuit (as bpgpu_r1cs_prover_session_polys_param), else NULL
 * Row r of prover p evaluates to e[p][r] = sum over the row's terms of coeff * value, the value of a `One` term being 1 and, for a
 * parametric circuit, coeff = c0 + sum_j chi_j c_j.  The coefficients are taken as the circuit was created with them: the minus that
 * the flattening puts on w_V and w_c is no part of a row.
 *   ok             nb x int32     1 iff first_bad_row and first_bad_gate are both -1
 *   first_bad_row  (optional) nb x int64   the smallest r with e[p][r] != 0, or -1
 *   first_bad_gate (optional) nb x int64   the smallest i with a_L[i] a_R[i] != a_O[i], or -1.  The reference has no such test: its
 *                                 Prover::multiply / allocate_multiplier compute a_O themselves.  Here a_O crosses the ABI, so the
 *                                 check covers it.
 *   residuals      (optional) nb x q x 32  canonical LE: e itself, for a caller that debugs a gadget; NULL: nothing per row is stored
 * The row-major view of the circuit that these calls evaluate is built on the device the first time one of them (or
 * bpgpu_mpc_constraints_eval) sees the handle -- that first call waits for the build, also in the `_dev` form -- and lives in the handle
 * until bpgpu_circuit_destroy; bpgpu_circuit_create* costs what it did for callers that never ask.  A handle may be checked from
 * several contexts of its device at once.
 * Refusals, before anything is launched: BPGPU_E_ARG for a null required pointer, for gadget challenges given to a numeric circuit or
 * missing for a parametric one; BPGPU_E_LEN for n or m above 2^25 - 1; nb == 0: BPGPU_OK.  A non-canonical limb gives BPGPU_E_ARG in
 * the host form and raises bpgpu_input_flag in the `_dev` form (every operand and result a device pointer; asynchronous on the
 * context's stream).  A failed call leaves no pool memory behind. */
int bpgpu_r1cs_constraints_satisfied(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *a_L, const uint8_t *a_R,
                                     const uint8_t *a_O, const uint8_t *v, const uint8_t *gadget_challenges, int32_t *ok,
                                     int64_t *first_bad_row, int64_t *first_bad_gate, uint8_t *residuals);
int bpgpu_r1cs_constraints_satisfied_dev(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const void *a_L, const void *a_R,
                                         const void *a_O, const void *v, const void *gadget_challenges, void *ok, void *first_bad_row,
                                         void *first_bad_gate, void *residuals);
/* ---- witness synthesis: Prover::multiply (r1cs/prover.rs:99-125) and allocate_multiplier (:148-165) on the device ----------------------
 * A bpgpu_witness is a resident GATE PROGRAM: how the n multipliers of one prover are assigned, in order, the first n1 of them in
 * phase 1.  Gate i has an op (op[i]), an argument (arg[i]) and two rows, 2i = `left` and 2i + 1 = `right`, in the CSR of
 * bpgpu_circuit_create_param: kinds 0..4, (1 + nchi) * 2n stored rows, block j >= 1 holding the chi_j parts (a coefficient is
 * c0 + sum_j chi_j c_j), coefficients canonical little-endian.
 *   BPGPU_GATE_MUL    multiply(left, right): a_L[i] = eval(left), a_R[i] = eval(right), a_O[i] = a_L[i] a_R[i].  A term may read a
 *                     committed value (kind 3), One (kind 4) or a_L / a_R / a_O (kinds 0..2) of a gate < i.
 *   BPGPU_GATE_INPUT  allocate_multiplier(Some((l, r))), or a pair of allocate calls: (l, r) is the next pair of the caller's `inputs`
 *                     (nb x n_inputs x 2, ark form), consumed in gate order; a_O = l r.  Both rows must be empty.
 *   BPGPU_GATE_BIT    the range gadget's assignment (tests/r1cs.rs:629-632): b = bit arg[i] of the canonical integer eval(left);
 *                     a_L = 1 - b, a_R = b, a_O = a_L a_R.  The right row must be empty.  arg[i] < 252: the reference's u64
 *                     assignment, generalised to the whole field.
 *   BPGPU_GATE_INV    inverse-or-zero, the allocate_multiplier(Some((x, x^-1))) of an is-zero / equality / not-equal gadget or of a
 *                     division: a_L[i] = eval(left); a_R[i] = a_L[i]^-1, or 0 when a_L[i] = 0; a_O[i] = a_L[i] a_R[i], so a_O is 1 for
 *                     a non-zero a_L and 0 for zero.  The zero test is on the canonical integer of eval(left).  The right row must be
 *                     empty; arg[i] is ignored; the left row may hold whatever a MUL row may.  In the block and scan forms the INV
 *                     gates of a level share ONE inversion per thread (Montgomery's trick, csrc/witness_dev.cuh); a lane, and a
 *                     wave that sums a row of more than 64 terms, invert once per gate.  An INV gate has the level of a MUL gate
 *                     with its left row, is never a chain MEMBER of either kind, may be a chain's head, and a MUL may link to its
 *                     a_O.  A phase without an INV gate launches the kernels it always did.  Measured (profiles/witness_inv.log,
 *                     median ms; block form | lane form | the same program with INPUT gates handed the pairs, the host's work
 *                     left out): 256 provers x one level of 1024 INV gates 0.123 | 45.964 | 0.074; 1 x 1024: 0.093 | 50.777 |
 *                     0.045; 4096 x 16: 0.634 | 0.743 | 0.055; 256 x a chain of 64, one gate a level, nothing to batch: 3.102 |
 *                     2.921 | 0.031.  Every other shape is UNMEASURED; the route rule is the one below, unchanged.
 *   BPGPU_GATE_DIVREM the integer quotient and remainder of a div-rem / floor gadget, its allocate(Some(q)) and allocate(Some(r)),
 *                     which share one multiplier (prover.rs:127-146): with x and y the CANONICAL integers in [0, n) of eval(left)
 *                     and eval(right), a_L[i] = floor(x / y), a_R[i] = x mod y, a_O[i] = a_L[i] a_R[i] mod n; for y = 0 (an empty
 *                     right row is one) a_L[i] = 0 and a_R[i] = x.  x = a_L[i] y + a_R[i] holds over the integers for every input:
 *                     it is the circuit's range check r < y that rejects a zero divisor.  Both rows may hold whatever a MUL row
 *                     may; arg[i] is ignored; validation is that of a MUL gate with the same rows.  The division is a restoring
 *                     shift-and-subtract on 8 x 32-bit words (csrc/int_div.cuh), bitlen(x) - bitlen(y) + 1 steps, none for x < y.
 *                     A DIVREM gate has the level of a MUL gate with its rows, is never a chain MEMBER of either kind, may be a
 *                     chain's head, and a MUL may link to its a_O; in the block and scan forms it is strided over the threads
 *                     like any gate of its level (nothing is batched), and for a row of more than 64 terms lane 0 divides what
 *                     the wave summed.  A phase without a DIVREM gate launches the kernels it always did.
 *                     Measured (profiles/witness_divrem.log, median ms; block form | lane form | the same program with
 *                     INPUT gates handed the (q, r) pairs in the block form | in the lane form, the host's work left out; x of 64
 *                     bits over y of 33 bits, then x of 252 bits over y of 128 bits): 256 provers x one level of 1024 DIVREM
 *                     gates 0.101 | 12.917 | 0.074 | 5.565, then 0.138 | 21.593 | 0.075 | 5.580; 1 x 1024: 0.072 | 13.449 | 0.045 |
 *                     5.767, then 0.107 | 22.789 | 0.045 | 5.660; 4096 x 16: 0.079 | 0.225 | 0.055 | 0.116, then 0.117 | 0.360 |
 *                     0.055 | 0.116; 256 x a chain of 64, one gate a level: 1.061 | 0.861 | 0.031 | 0.371, then 1.810 | 1.402 |
 *                     0.031 | 0.371.  Every other shape is UNMEASURED; the route rule is the one below, unchanged.
 * bpgpu_witness_create validates on the host, before anything is uploaded; after it no kernel index can be out of range.
 * BPGPU_E_ARG: a null pointer, an unknown op or kind, a multiplier term with idx >= i (a self or forward reference), a chi part in a
 * gate < n1 (the challenge does not exist in phase 1), a committed index >= m, a BIT with arg >= 252, a non-empty row where the op
 * requires an empty one, row pointers that decrease, a non-canonical coefficient, n1 > n, nchi > 8.  BPGPU_E_LEN: n or m above 2^25 - 1.
 * It also computes the dependency levels, per phase: a gate's level is 0 if it is an INPUT or its rows read no multiplier of its
 * own phase, else 1 + the largest level it reads; the gates of a phase are stored sorted by level.
 * Three launch forms evaluate a phase, one launch each (csrc/k_witness.hip): a LANE per prover walks the gates in program order; a
 * BLOCK per prover walks the levels, a level's gates strided over 256 threads and a row of more than 64 terms summed by a wave; the
 * SCAN form is the block form over compressed levels, with every product chain evaluated as a prefix product.
 * A product chain is recognised from the program's shape alone.  Gate i of a phase is a MEMBER with predecessor j when it is a
 * BPGPU_GATE_MUL, one of its rows (the left is tried first) is the LINK row -- exactly one stored term over all 1 + nchi blocks (an
 * explicit zero coefficient is a term), of kind 2 on a gate j of the same phase that has no member successor yet (of two gates linking
 * to one a_O the first in program order is the member) -- and the other, FREE row has no term of kind 0..2 on a gate of the same
 * phase.  A gate with a successor and no predecessor is the chain's HEAD (any op, any rows).  Along a chain a_O is a prefix product of
 * factors that read nothing of their phase, and F_n multiplication is exactly associative on canonical values: a 256-thread block
 * scans all chains headed at one level together (segmented, no inversion: a zero factor zeroes the rest of its chain) in about
 * 2 ceil(M / 256) + 10 dependent multiplications for M members, and stores the bytes the gates one by one give.  In the compressed
 * levels a member takes its predecessor's level.  bpgpu_witness_chains reports the chains, and product chains only.
 * A second pass over the program, once every product member is known, finds the AFFINE chains.  In program order, a BPGPU_GATE_MUL
 * that pass 1 left without a predecessor is an affine member with predecessor j when one of its rows (the left is tried first) is
 * an affine LINK row -- it holds exactly ONE stored term, over all 1 + nchi blocks, of kind 0..2 on a gate of the same phase; that
 * term is of kind 2, on a gate j that has no member successor of either kind yet (a product gate keeps its a_O whatever the order);
 * beside it the row may hold any number of terms that read nothing of the phase: committed values, One, multipliers of phase 1 in a
 * phase-2 gate, with or without chi parts -- and the other row is free as above.  An explicit zero coefficient is still a term, and
 * a link coefficient split over two blocks (c0 + chi c1 on the same a_O[j]) is TWO terms: that gate stays ordinary.  With the link
 * row c a_O[j] + f and the free row g, a_O[i] = (c g) a_O[j] + f g: the affine map x -> A x + B with A = c g, B = f g, and a product
 * member is the map with f = 0.  Affine maps compose associatively, (A2, B2) o (A1, B1) = (A2 A1, A2 B1 + B2), so the EXTENDED chains
 * -- product and affine members in any order; a gate that pass 1 called a head may become a member -- are evaluated by the same scan
 * as a segmented prefix composition, in the same number of steps, and store the bytes the gates one by one give (a zero g leaves B
 * alone for the rest of its chain).  This covers Horner evaluation of committed vectors at a challenge, running sums scaled by a
 * challenge factor, any accumulate-then-multiply loop.  In the extended compressed levels a member of either kind takes its
 * predecessor's level; a phase that has an affine member is scanned over those.  bpgpu_witness_affine_chains reports them.
 * What is still serial, one level per gate: a gate both of whose rows read its phase (a squaring, the x^5 of a Poseidon round), a
 * link through a_L or a_R, and a link coefficient split over blocks.
 * The route is a function of the program's shape and nb alone, never of the data: bpgpu_witness_plan (no device needed) reports
 * what the library takes.  A phase takes the scan form when its longest product chain has BPGPU_OPT_WITNESS_SCAN_MIN members or more,
 * or when its longest extended chain has max(BPGPU_OPT_WITNESS_SCAN_MIN, 16) members or more (the 16 by the rule below on Horner
 * gadgets of 8 .. 16 382 members, profiles/witness_affine.log: at 16 members 0.053 against 0.176 ms for 1 prover and 0.061 against
 * 0.215 ms for 256, more provers UNMEASURED; BPGPU_OPT_WITNESS_SCAN_MIN 1 scans every chain of either kind, 0 none).  For product chains the
 * default, 16, is the smallest power of two >= 16 from which on the scan form's slowest step lay below the block form's fastest for 1
 * and for 256 provers (profiles/witness_synth.log, chains of 8 .. 16 382 members; at 16 members 0.053 against 0.200 ms and 0.058
 * against 0.222 ms), and 4096 provers of the 64-shuffle (62 members) take 0.273 ms scanned, 1.273 ms on lanes, 3.217 ms in blocks;
 * shorter chains above 256 provers, and any chain above 4096 provers, are UNMEASURED.  Otherwise: the block form where a level
 * holds two gates or more on average, for up to 1024 provers (measured: the same log, DESIGN.md "Witness synthesis"); above that
 * the width asked for grows with nb / 1024, which is an extrapolation and UNMEASURED.  BPGPU_OPT_WITNESS_ROUTE 1 or 2 forces a form
 * (the scan form cannot be forced, only enabled: BPGPU_OPT_WITNESS_SCAN_MIN 1 scans every chain, 0 none; the environment seeds of a
 * new context are BPGPU_WITNESS_ROUTE and BPGPU_WITNESS_SCAN_MIN); results never depend on either. */
typedef struct bpgpu_witness bpgpu_witness;
#define BPGPU_GATE_MUL 0
#define BPGPU_GATE_INPUT 1
#define BPGPU_GATE_BIT 2
#define BPGPU_GATE_INV 4 /* not 3: callers and tests probe 3 as "an unknown op", so 3 stays refused (BPGPU_E_ARG) */
#define BPGPU_GATE_DIVREM 6 /* not 5: tests probe 5 as "an unknown op" too, so 5 stays refused, like 3 and every op above 6 */
int bpgpu_witness_create(bpgpu_ctx *ctx, size_t n, size_t n1, size_t m, size_t nchi, const uint8_t *op, const uint32_t *arg,
                         const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx, const uint8_t *coeff, bpgpu_witness **out);
void bpgpu_witness_destroy(bpgpu_ctx *ctx, bpgpu_witness *w);
#define BPGPU_WIT_PLAN_LEVELS1 0      /* dependency levels of phase 1 (0: no gates) */
#define BPGPU_WIT_PLAN_LEVELS2 1      /* ... of phase 2 */
#define BPGPU_WIT_PLAN_WIDEST 2       /* gates of the widest level of either phase */
#define BPGPU_WIT_PLAN_LONG_ROWS 3    /* rows of more than 64 terms (a wave's in the block form) */
#define BPGPU_WIT_PLAN_INPUTS 4       /* INPUT gates: pairs of `inputs` per prover */
#define BPGPU_WIT_PLAN_ROUTE1 5       /* launch form of phase 1: 1 = a lane per prover, 2 = a block per prover, 3 = a block per prover with
                                       * the product and affine chains scanned (at the default BPGPU_OPT_WITNESS_SCAN_MIN); 0: no gates */
#define BPGPU_WIT_PLAN_ROUTE2 6       /* ... of phase 2 */
#define BPGPU_WIT_PLAN_FIELDS 7
int bpgpu_witness_plan(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                       const uint32_t *idx, size_t nb, int32_t out[BPGPU_WIT_PLAN_FIELDS]);
/* The product chains of a gate program, from its shape alone (no device needed): per phase the number of chains, of their members, the
 * members of the longest one and the COMPRESSED levels the scan form walks.  Refusals: those of bpgpu_witness_plan. */
#define BPGPU_WIT_CHAIN_CHAINS1 0
#define BPGPU_WIT_CHAIN_CHAINS2 1
#define BPGPU_WIT_CHAIN_MEMBERS1 2
#define BPGPU_WIT_CHAIN_MEMBERS2 3
#define BPGPU_WIT_CHAIN_LONGEST1 4
#define BPGPU_WIT_CHAIN_LONGEST2 5
#define BPGPU_WIT_CHAIN_LEVELS1 6
#define BPGPU_WIT_CHAIN_LEVELS2 7
#define BPGPU_WIT_CHAIN_FIELDS 8
int bpgpu_witness_chains(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                         const uint32_t *idx, int32_t out[BPGPU_WIT_CHAIN_FIELDS]);
/* The EXTENDED chains of a gate program -- product and affine members together ("affine member" above) -- from its shape alone (no
 * device needed): per phase the number of chains, of all their members, of the members that pass 2 added (the affine ones), the
 * members of the longest chain and the extended compressed levels, which the scan form walks.  A program without an affine member
 * reports the figures of bpgpu_witness_chains.  Refusals: those of bpgpu_witness_plan. */
#define BPGPU_WIT_AFF_CHAINS1 0
#define BPGPU_WIT_AFF_CHAINS2 1
#define BPGPU_WIT_AFF_MEMBERS1 2
#define BPGPU_WIT_AFF_MEMBERS2 3
#define BPGPU_WIT_AFF_AFFINE1 4
#define BPGPU_WIT_AFF_AFFINE2 5
#define BPGPU_WIT_AFF_LONGEST1 6
#define BPGPU_WIT_AFF_LONGEST2 7
#define BPGPU_WIT_AFF_LEVELS1 8
#define BPGPU_WIT_AFF_LEVELS2 9
#define BPGPU_WIT_AFF_FIELDS 10
int bpgpu_witness_affine_chains(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                                const uint32_t *idx, int32_t out[BPGPU_WIT_AFF_FIELDS]);
/* The witnesses of nb provers of one gate program, where the provers read them.
 *   v                  nb x m          the committed values, ark form: the buffer bpgpu_r1cs_commit_values and
 *                                      bpgpu_r1cs_constraints_satisfied take; may be NULL when m == 0
 *   inputs             nb x n_inputs x 2   ark form; may be NULL when the program has no INPUT gate (phase 2 of a program consumes the
 *                                      pairs that follow those of phase 1)
 *   gadget_challenges  nb x nchi x 32  canonical LE, for a program with nchi > 0 when phase 2 is evaluated (phase 0 or 2), else NULL
 *   phase              0: all gates; 1: gates [0, n1); 2: gates [n1, n), the planes already holding phase 1
 *   a_L, a_R, a_O      nb x n          ark form: the layouts bpgpu_r1cs_constraints_satisfied and bpgpu_r1cs_prove_fs take, so one set of
 *                                      device buffers serves commit -> synthesize -> check -> prove without a host wait.  The host form
 *                                      of phase 1 or 2 copies the planes in and out whole: the other phase's multipliers come back as
 *                                      the caller held them.
 * Refusals, before any launch: BPGPU_E_ARG for a null required pointer, for challenges given to a numeric program or where phase 1
 * alone is evaluated, for challenges missing where a parametric program's phase 2 is, for a phase other than 0, 1, 2; nb == 0: BPGPU_OK,
 * nothing touched.  A non-canonical limb gives BPGPU_E_ARG in the host form and raises bpgpu_input_flag in the `_dev` form (every
 * operand a device pointer; asynchronous on the context's stream).  A failed call leaves no pool memory behind.  Profiling: kind 22.
 * A dependent gate costs the device about 10 us (a store, a load and a few dozen dependent multiplications of one lane), but a chain
 * of pure products is no longer serial: ONE prover's k = 2^14 shuffle, two chains of 16 382 members, takes 1.470 ms scanned
 * (profiles/witness_synth.log) where the block form takes 186 ms and an interpreted host 54 ms, and one 2^10-shuffle prover is proved
 * by bpgpu_r1cs_prove_fs2 in 4.7 ms against 10.1 ms for bpgpu_r1cs_prove_fs2_begin / _finish around that host's gadget.  Batches: 256
 * provers of the 64-shuffle in 0.057 ms, of 16 x 64-bit range values in 0.07 ms.  An accumulate-then-multiply chain such as
 * (a_O[i - 1] + v) w is an affine chain and scanned as well: ONE prover's Horner evaluation of two committed vectors of 2^14 values,
 * two chains of 16 382 affine members, takes 1.913 ms where the block form takes 165 ms and that host 50 ms
 * (profiles/witness_affine.log).  What is still serial is a chain of gates both of whose rows read their phase (a squaring, the x^5
 * of a Poseidon round), a link through a_L or a_R, or a link coefficient split over blocks: a caller with few provers and long chains
 * of THAT kind keeps its host's Prover::multiply.
 * Out of scope: the host mirror (mpc_bulletproof.hpp: its multiply keeps evaluating on the host), the pool forms (bpgpu_pool_*),
 * the two-party prover (a product of shares is a Beaver step, not a local product) and bench.py. */
int bpgpu_r1cs_witness_synthesize(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const uint8_t *v, const uint8_t *inputs,
                                  const uint8_t *gadget_challenges, uint8_t *a_L, uint8_t *a_R, uint8_t *a_O);
int bpgpu_r1cs_witness_synthesize_dev(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const void *v, const void *inputs,
                                      const void *gadget_challenges, void *a_L, void *a_R, void *a_O);
/* Prover::prove for nb provers of ONE two-phase circuit in ONE call: the phase-1 gates of w, the chain of bpgpu_r1cs_prove_fs2_begin,
 * the phase-2 gates on the gadget challenge that chain has just drawn (read from the session's device copy), the chain of
 * bpgpu_r1cs_prove_fs2_finish -- all on the context's stream, no host wait, no session left behind.  The launches of the two chains
 * are the ones _begin and _finish issue (the same code); outputs are byte-identical to that pair fed the host-evaluated witness.
 *   states_in, gadget_label   as bpgpu_r1cs_prove_fs2_begin (the label is host memory in both forms; NULL with attached labels)
 *   v, inputs       as bpgpu_r1cs_witness_synthesize
 *   s_L, s_R        nb x n, explicit blinding vectors (phase 1: [0, n1), phase 2: [n1, n) of each prover's row), or both NULL with
 *   vector_keys     nb x 2 x 32: a phase-1 key, then a phase-2 key (exactly one of the two sources)
 *   v_blinding      nb x m, ark form; may be NULL when m == 0
 *   blindings       nb x 11, ark form: i1 o1 s1 | i2 o2 s2 tb1 tb3 tb4 tb5 tb6
 *   proof_points, proof_scalars, wire, challenges_out, states_out   as bpgpu_r1cs_prove_fs2_finish
 *   gadget_challenges_out   (optional) nb x nchi x 32 canonical LE, prover-major
 *   a_L_out, a_R_out, a_O_out   (optional, all three or none) nb x n, ark form: the synthesized witness, e.g. for
 *                                      bpgpu_r1cs_constraints_satisfied afterwards
 * Refusals, before anything is launched: those of _begin and _finish; BPGPU_E_ARG for a null program, for a program whose
 * (n, n1, m, nchi) are not the circuit's, for nchi != 1, for a program with INPUT gates and no `inputs`.  A non-canonical ark limb gives
 * BPGPU_E_ARG in the host form and raises bpgpu_input_flag in the `_dev` form.  A failed call leaves no session or pool memory behind. */
int bpgpu_r1cs_prove_fs2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                         const uint8_t *states_in, const uint8_t gadget_label[32], const uint8_t *v, const uint8_t *inputs, const uint8_t *s_L,
                         const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *v_blinding, const uint8_t *blindings,
                         uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out,
                         uint8_t *gadget_challenges_out, uint8_t *a_L_out, uint8_t *a_R_out, uint8_t *a_O_out);
int bpgpu_r1cs_prove_fs2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                             const void *states_in, const uint8_t gadget_label[32], const void *v, const void *inputs, const void *s_L,
                             const void *s_R, const void *vector_keys, const void *v_blinding, const void *blindings, void *proof_points,
                             void *proof_scalars, void *wire, void *challenges_out, void *states_out, void *gadget_challenges_out,
                             void *a_L_out, void *a_R_out, void *a_O_out);
/* Prove from COMMITTED VALUES in one call: what a prover has -- the transcript state at Prover::new, the values and their blindings, the
 * gadget's INPUT pairs, the blinding factors -- in; what it ships -- commitments, proofs and a verdict per prover -- out.  The stages are
 * the calls above (the same code, handed device pointers), all on the context's stream, no host wait between them, nothing left behind.
 * Two circuit shapes are accepted, and nothing else:
 *   ONE-PHASE  c numeric (bpgpu_circuit_create / _ark), w with nchi == 0 and n1 == n, gadget_label == NULL.  Stage order:
 *              1 bpgpu_r1cs_commit_values with the chain from init_states, 2 bpgpu_r1cs_witness_synthesize phase 0,
 *              3 bpgpu_r1cs_constraints_satisfied, 4 bpgpu_r1cs_prove_fs on the states that stage 1 produced.
 *   TWO-PHASE  c parametric with nchi == 1, w with the same (n, n1, m, nchi), gadget_label given (32 bytes, host memory in both forms);
 *              or c with attached labels (bpgpu_circuit_set_gadget_labels), any nchi, and gadget_label == NULL.
 *              Stage order: 1 bpgpu_r1cs_commit_values, 2 the bpgpu_r1cs_prove_fs2 chain, which synthesizes both phases and draws the
 *              gadget challenge, 3 bpgpu_r1cs_constraints_satisfied on the witness and the challenge that stage 2 left on the device.
 *              The check necessarily runs AFTER the proof here: the phase-2 witness does not exist before the challenge.
 * The witness planes, the chain states between stage 1 and the prover and the gadget challenge live in the context's pool memory for
 * the length of the call (in the caller's buffers where a_*_out / gadget_challenges_out are given).  The one host wait is inherited from
 * bpgpu_r1cs_constraints_satisfied: the first use of a circuit handle builds its row-major view, here before any stage is launched.
 * REJECTED PROVERS SHIP NOTHING.  After the last stage ONE launch (k_prove_fs.hip, profiling kind 22; the stages keep their kinds)
 * clears, for every prover with ok[p] == 0, its rows of proof_points, proof_scalars, wire, challenges_out and states_out to zero bytes:
 * an all-zero wire proof has version byte 0 and undecodable points, and every wire verifier rejects it.  V, V_compressed, ok,
 * first_bad_row, first_bad_gate, gadget_challenges_out and the witness outputs are left alone: they are the diagnostics.  Accepted
 * provers' bytes are untouched.  The host form and the `_dev` form behave the same; the `_dev` form never waits for ok.
 * Every operand has the encoding and layout of the call it is handed to:
 *   init_states, v, v_blinding, V, V_compressed   as bpgpu_r1cs_commit_values (init_states: its states_in; V, V_compressed optional)
 *   inputs                                         as bpgpu_r1cs_witness_synthesize
 *   ok, first_bad_row, first_bad_gate              as bpgpu_r1cs_constraints_satisfied (nb x int32; optional nb x int64 each)
 *   one-phase: s_L, s_R nb x n or vector_keys nb x 32, blindings nb x 8, proof_points, proof_scalars, wire, challenges_out, states_out
 *              as bpgpu_r1cs_prove_fs; gadget_challenges_out is not written
 *   two-phase: s_L, s_R nb x n or vector_keys nb x 2 x 32, blindings nb x 11, the results and gadget_challenges_out as bpgpu_r1cs_prove_fs2
 *   a_L_out, a_R_out, a_O_out                      (optional, all three or none) nb x n, ark form: the synthesized witness
 * For accepted provers every output equals, byte for byte, what the chain of the host-form calls returns on the same operands; for
 * rejected provers ok, first_bad_row, first_bad_gate, V and V_compressed do.  Results never depend on BPGPU_OPT_WITNESS_ROUTE,
 * BPGPU_OPT_WITNESS_SCAN_MIN or any other route option.
 * Refusals, all before anything is launched: those of the constituent calls, and BPGPU_E_ARG for a null ok, proof_points or
 * proof_scalars, for a null program, for a program whose (n, n1, m, nchi) are not the circuit's (a one-phase program has n1 == n), for
 * nchi > 1, for a label given to a one-phase pair or missing for a two-phase one, for a program with INPUT gates and no `inputs`, for
 * some but not all of the three witness outputs, for both or neither blinding-vector source and for a context after
 * bpgpu_set_shard(world > 1); BPGPU_E_LEN for n == 0, or n1 >= n in the two-phase shape; BPGPU_E_GENS for padded_n above the
 * generators' capacity; nb == 0: BPGPU_OK, nothing touched.  A non-canonical ark limb gives BPGPU_E_ARG in the host form and raises
 * bpgpu_input_flag in the `_dev` form (every operand and result but the label a device pointer; asynchronous on the context's stream).
 * A failed or refused call leaves no session and no pool memory behind.
 * Measured (profiles/prove_values.log: wall clock of a batch in host form on an MI355X, pageable memory, median (min..max) ms, the one
 * call | the chain of host-form calls it replaces, timed on a build of the parent commit; faster means the one call's maximum lies
 * below the chain's minimum): 256 provers x 16 x 64-bit range values (n = 1024, m = 16) 14.135 (14.048..14.202) | 15.932
 * (15.815..16.122), faster by 1.8 ms; 256 x shuffle 64 6.791 (6.774..6.836) | 7.466 (7.428..7.566), faster by 0.7 ms (from
 * page-locked memory 6.698 (6.666..7.100) | 6.983 (6.965..7.016): the spans overlap, nothing is claimed); ONE shuffle-2^10 prover
 * 33.272 (30.185..39.759) | 34.947 (30.998..40.040): the spans overlap, nothing is claimed; the range shape on a {0, 0} pool 13.761
 * (13.607..14.246) against 14.611 (14.353..14.939) for bpgpu_r1cs_witness_synthesize + bpgpu_pool_r1cs_prove_fs, which commit and
 * check nothing; the clearing launch at 256 provers 0.008 ms.  Every other shape is UNMEASURED. */
int bpgpu_r1cs_prove_values(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                            const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *v, const uint8_t *v_blinding,
                            const uint8_t *inputs, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *vector_keys, const uint8_t *blindings,
                            uint8_t *V, uint8_t *V_compressed, int32_t *ok, int64_t *first_bad_row, int64_t *first_bad_gate,
                            uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out,
                            uint8_t *gadget_challenges_out, uint8_t *a_L_out, uint8_t *a_R_out, uint8_t *a_O_out);
int bpgpu_r1cs_prove_values_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, const bpgpu_witness *w, size_t nb,
                                const void *init_states, const uint8_t gadget_label[32], const void *v, const void *v_blinding,
                                const void *inputs, const void *s_L, const void *s_R, const void *vector_keys, const void *blindings, void *V,
                                void *V_compressed, void *ok, void *first_bad_row, void *first_bad_gate, void *proof_points, void *proof_scalars,
                                void *wire, void *challenges_out, void *states_out, void *gadget_challenges_out, void *a_L_out, void *a_R_out,
                                void *a_O_out);
/* ---- two-party prover: ONE party's local arithmetic (src/r1cs_mpc/: the collaborative prover over SPDZ-style shares) ----------------
 * An authenticated scalar held by party p is THREE planes: a share s_p, a MAC share m_p and a public modifier c, identical at both
 * parties.  Invariants: value v = s_0 + s_1 + c; m_0 + m_1 = alpha (s_0 + s_1), alpha = alpha_0 + alpha_1 the MAC key.  No local step
 * needs the party index or alpha: a public constant is added to c only; a public factor scales all three planes; two values add plane
 * by plane; a product a b of two shared values uses a triple (x, y, z = x y): the parties open d = a - x and e = b - y, then the
 * product's planes are z_k + d y_k + e x_k (k = share, MAC, modifier) plus d e on the modifier plane.  A point (an MSM over a plane)
 * opens as the sum of the parties' share points plus the modifier point.  (A host whose library keeps public constants inside party
 * 0's share maps onto this at the boundary: INTEGRATION.md.)
 * Encodings: every share, MAC, modifier, triple, masked and opened value -- inputs and outputs -- is in ark-ff Montgomery form
 * (x 2^256 mod n, 4 little-endian u64), which is additive, so a host adds the parties' masked planes without converting them;
 * challenges y, z, x, u, w, the IPP's u and u^-1 and the gadget challenges are 32-byte canonical little endian, once per proof (the
 * library broadcasts them to the planes); points are 64-byte x || y; wV is canonical little endian (public).
 * Layouts, proof-major; "3" is the plane (share, MAC, modifier), len the length of the step's vectors:
 *   operand vectors  nb x 3 x n_new                 blindings      nb x 3 x 3 (i, o, s blinding)
 *   triples          nb x J x 3 (x, y, z) x 3 x len  masked         nb x J x 2 (d, e) x 3 x len     opened   nb x J x 2 (d, e) x len
 *   where J = 6 products of the polynomial build (l1 r1, l2 r1, l3 r1, l1 r3, l2 r3, l3 r3; len = n) or 2 of an IPP round (c_L =
 *   <a_L, b_R>, c_R = <a_R, b_L>; len = bpgpu_ipp_len / 2); an opened value is d (or e) summed over both parties' share planes plus
 *   the modifier plane.
 * Each call ends where the reference opens something over the network.  Shape errors (a missing pointer, s_L / s_R, gadget challenges
 * given to a numeric circuit or missing for a parametric one, a call out of order, a context after bpgpu_set_shard) give BPGPU_E_ARG,
 * a circuit whose multipliers are not the session's BPGPU_E_LEN, before anything is launched; a non-canonical limb in any input
 * gives BPGPU_E_ARG as the single-party session calls do.  The single-party calls refuse these sessions (BPGPU_E_ARG):
 * bpgpu_r1cs_prover_commit / _eval / _session_polys(_param) / _ipp_begin, bpgpu_ipp_round and bpgpu_ipp_run_fs.
 *
 * bpgpu_mpc_prover_commit -- mpc_prover.rs:621-657 (first call, *session == NULL) and :717-750 (second call: the n_new phase-2
 *   multipliers): the authenticated bpgpu_r1cs_prover_commit.  s_L, s_R explicit (blinding vector keys have no place: the fabric
 *   deals shared blindings).  commitments out: nb x 3 x 3 x 64 B (proof, plane, A_I A_O S).
 * bpgpu_mpc_prover_polys_mask -- mpc_prover.rs:783-829 and the masking half of authenticated_poly.rs:143-164: y^-1, the flattened
 *   constraints, l1 = a_L + y^-i wR, l2 = a_O, l3 = s_L, r0 = wO - y^i (public), r1 = y^i a_R + wL, r3 = y^i s_R per plane (public
 *   terms on the modifier plane), and masked (nb x 6 x 2 x 3 x n) for the six shared x shared products from triples (nb x 6 x 3 x 3
 *   x n: 6n triples per proof).  gadget_challenges: nb x nchi x 32 B for a circuit of bpgpu_circuit_create_param, else NULL.
 * bpgpu_mpc_prover_polys_finish -- the combine half of special_inner_product and mpc_prover.rs:836-864: opened (nb x 6 x 2 x n) ->
 *   t_coeffs out nb x 3 x 6 (proof, plane, t1..t6), the products with the public r0 computed locally; t_blindings nb x 3 x 5 (tb1,
 *   tb3, tb4, tb5, tb6) -> T out nb x 3 x 5 x 64 B (T_1, T_3..T_6 per plane); wV out nb x m (canonical) for the host's t_2_blinding.
 * bpgpu_mpc_prover_ipp_begin -- mpc_prover.rs:901-917 and the set-up of SharedInnerProductProof::create: l(x), r(x) per plane (the
 *   -y^i padding on the modifier plane), G / H factors, Q = w B over the resident generators.  x, u, w: nb x 32 B.
 * Per round while bpgpu_ipp_len(ipp) > 1 (mpc_inner_product.rs:52-228):
 *   bpgpu_mpc_ipp_mask  -- triples nb x 2 x 3 x 3 x h -> masked nb x 2 x 2 x 3 x h for c_L, c_R   (h = bpgpu_ipp_len / 2)
 *   bpgpu_mpc_ipp_round -- opened nb x 2 x 2 x h -> L, R: nb x 3 x 64 B each (c_L Q, c_R Q from the Beaver combine)
 *   bpgpu_ipp_fold      -- u, u^-1: nb x 32 B (once per proof), applied to all planes
 * then bpgpu_ipp_finish -> a, b: nb x 3 x 32 B each, ark-ff Montgomery form.  2 (padded_n - 1) triples per proof over all rounds. */
int bpgpu_mpc_prover_commit(bpgpu_ctx *ctx, const bpgpu_gens *g, bpgpu_prover **session, size_t nb, size_t n_new, const uint8_t *a_L,
                            const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R, const uint8_t *blindings,
                            uint8_t *commitments);
int bpgpu_mpc_prover_polys_mask(bpgpu_ctx *ctx, bpgpu_prover *session, const bpgpu_circuit *c, const uint8_t *y, const uint8_t *z,
                                const uint8_t *gadget_challenges, const uint8_t *triples, uint8_t *masked);
int bpgpu_mpc_prover_polys_finish(bpgpu_ctx *ctx, bpgpu_prover *session, const uint8_t *opened, const uint8_t *t_blindings,
                                  uint8_t *t_coeffs, uint8_t *T, uint8_t *wV);
int bpgpu_mpc_prover_ipp_begin(bpgpu_ctx *ctx, bpgpu_prover *session, const bpgpu_gens *g, size_t padded_n, size_t n1, const uint8_t *x,
                               const uint8_t *u, const uint8_t *w, bpgpu_ipp **out);
int bpgpu_mpc_ipp_mask(bpgpu_ctx *ctx, bpgpu_ipp *ipp, const uint8_t *triples, uint8_t *masked);
int bpgpu_mpc_ipp_round(bpgpu_ctx *ctx, bpgpu_ipp *ipp, const uint8_t *opened, uint8_t *L, uint8_t *R);
/* bpgpu_mpc_constraints_eval -- one party's local half of MpcProver::constraints_satisfied (mpc_prover.rs:556-568), which evaluates
 * every row on shares and opens them in one batch: a_L, a_R, a_O nb x 3 x n and v nb x 3 x m (the committed values' planes; NULL when
 * m == 0) in the plane layout above, gadget_challenges nb x nchi x 32 B canonical LE for a parametric circuit, else NULL ->
 * residuals nb x 3 x q, ark form: row r on plane k of proof p at [(3 p + k) q + r].  Every plane is evaluated alike; the constant of a
 * `One` term goes to the modifier plane only (the rule for public constants above).  The host opens the planes (open_batch) and
 * compares with zero.  The gate identity a_L a_R = a_O is NOT checked: on shares it is a Beaver product, which needs a triple and an
 * opening of its own -- the fabric's business.  Refusals and the circuit's row-major view: as bpgpu_r1cs_constraints_satisfied. */
int bpgpu_mpc_constraints_eval(bpgpu_ctx *ctx, const bpgpu_circuit *c, size_t nb, const uint8_t *a_L, const uint8_t *a_R,
                               const uint8_t *a_O, const uint8_t *v, const uint8_t *gadget_challenges, uint8_t *residuals);
/* bpgpu_mpc_commit_values -- one party's local half of MpcProver::commit_preshared / batch_commit_preshared (mpc_prover.rs:402-456;
 * PedersenGens::commit_shared, generators.rs:52-58): v, v_blinding nb x 3 x m in the plane layout above, ark form -> V nb x 3 x m x 64 B,
 * V_k = v_k B + v_blinding_k B_blinding on every plane alike over g's resident Pedersen pair; no step needs the party index.  There is
 * no transcript: the parties open the points over the network first, and the host absorbs the OPENED values.  Shape and limb errors as
 * bpgpu_r1cs_commit_values (a null V is "no output"; BPGPU_E_LEN for 3 nb m above 2^30). */
int bpgpu_mpc_commit_values(bpgpu_ctx *ctx, const bpgpu_gens *g, size_t nb, size_t m, const uint8_t *v, const uint8_t *v_blinding,
                            uint8_t *V);
/* ---- two-party witness synthesis: MpcProver::multiply / allocate_multiplier (r1cs_mpc/mpc_prover.rs:183-282) level by level --------
 * The two-party prover now has its own calls for the witness: a bpgpu_witness gate program (above) is evaluated on three-plane shares,
 * one DEPENDENCY LEVEL at a time.  The gates of one level read only lower levels, so they are independent, and the product of every
 * gate is a Beaver step that needs an opening: one level is one network round.  Per level the host calls _mask, opens d and e of
 * every gate of the level (the opening and its MAC check are the fabric's), and calls _combine.  The product and affine scans of the
 * single-party path do not carry over: the level is the unit.
 *   bpgpu_witness_gate_levels  level[i] of gate i inside its phase (0 for an INPUT gate or a gate whose rows read no multiplier of its
 *       own phase, else 1 + the largest level read): the definition bpgpu_witness_create already uses.  No device.  Refusals: those of
 *       bpgpu_witness_plan, and BPGPU_E_ARG for a null `level` with n > 0.  A host learns from it, before a session exists, which gate
 *       element t of a round belongs to and how many triples each round needs.
 * Encodings and plane rules are those of "two-party prover" above: every share, MAC, modifier, triple, masked and opened value is in
 * ark-ff Montgomery form; gadget challenges are canonical little-endian, one set per proof, and public: a coefficient
 * c0 + sum_j chi_j c_j scales all three planes alike.  Layouts, proof-major, "3" the plane (share, MAC, modifier):
 *   v                  nb x 3 x m             may be NULL when m == 0
 *   inputs             nb x 3 x n_inputs x 2  all pairs of the program (phase 2 consumes those after phase 1's); may be NULL when the
 *                                             program has no INPUT gate
 *   a_L, a_R, a_O      nb x 3 x n             _begin reads them only for phase == 2, where they hold phase 1 (NULL otherwise); _finish
 *                                             writes all of them: the other phase's multipliers come back as given, zero if never given
 *   phase              0, 1 or 2, with the meaning, and the rules for gadget_challenges, of bpgpu_r1cs_witness_synthesize
 * One level, with G = bpgpu_mpc_witness_level_len (the gates of the level the next _mask evaluates; 0 when none is left):
 *   triples  nb x 3 (x, y, z) x 3 x G       masked  nb x 2 (d, e) x 3 x G       opened  nb x 2 (d, e) x G
 * Element t belongs to the t-th gate of that level in ascending gate index.
 *   _mask     for every gate i of the level and every plane k: a_L[i] = the left row evaluated on plane k -- a `One` term contributes
 *             its coefficient on the modifier plane only and nothing on the other two, as bpgpu_mpc_constraints_eval does -- and
 *             a_R[i] likewise from the right row; an INPUT gate takes the next pair's planes.  The results are stored in the
 *             session, d = a_L - x and e = a_R - y are written per plane, and the session keeps the triples.
 *   _combine  a_O[i] on plane k = z_k + d y_k + e x_k, plus d e on the modifier plane; then the session advances to the next level.
 *             Every gate takes a triple, also one whose row happens to be public, because the reference's &l * &r does.
 * Rounds: one _mask / _combine pair per level, so the number of openings is the phase's level count (BPGPU_WIT_PLAN_LEVELS1 /
 * BPGPU_WIT_PLAN_LEVELS2, both for phase 0); bpgpu_mpc_witness_levels_left counts them down.  A phase without gates has zero levels:
 * _begin succeeds and _finish returns the planes unchanged.  The program handle must outlive the session.
 * Refusals, all before anything is launched.  BPGPU_E_ARG: a null required pointer; a phase other than 0, 1 or 2; challenges given or
 * missing against the rules of bpgpu_r1cs_witness_synthesize; planes missing for phase 2; a BPGPU_GATE_BIT gate in the evaluated
 * phase (a bit of a shared value is not a local function: the range gadget on shares takes its bits as INPUT pairs (1 - b, b)); a
 * BPGPU_GATE_INV gate in the evaluated phase (neither is the inverse of a shared value: on shares the is-zero gadget takes
 * (x, x^-1) as an INPUT pair; a phase without one is evaluated as before, whatever the other phase holds); a
 * BPGPU_GATE_DIVREM gate in the evaluated phase (nor is the integer quotient of a shared value: on shares the div-rem gadget takes
 * (q, r) as an INPUT pair; again a phase without one is evaluated as before); a
 * context after bpgpu_set_shard(world > 1); _mask twice in a row; _combine without a _mask; _mask with no level left; _finish with a
 * level left.  BPGPU_E_LEN: 3 nb n or 3 nb m above 2^30.  nb == 0: BPGPU_OK with *out left NULL.  A non-canonical ark limb in any
 * input, `opened` and `triples` included, gives BPGPU_E_ARG, as the other two-party calls do; the session stays where it was (the
 * call may be repeated with good operands, or the session destroyed).  A failed call leaves no pool memory behind;
 * bpgpu_mpc_witness_destroy frees an abandoned session (and a finished one: _finish does not).  Profiling: kind 22.
 * Launches (csrc/k_mpc_witness.hip): _mask is one launch over (virtual prover 3 p + k, gate of the level), a lane per gate and a wave
 * per gate with a row of more than 64 stored terms; _combine one launch, a lane per (virtual prover, gate).  Measured
 * (profiles/mpc_witness.log, tools/bench_mpc_witness.py: the device part of ONE _mask + _combine pair of one party under the
 * library's own events, kind 22 -- the conversions of triples, masked and opened values included, the host's copies and waits not):
 * 1.957 ms for 256 proofs of one level of 1 024 INPUT gates, 0.073 ms per level for 256 proofs of the 64-shuffle (63 levels of 2
 * gates), 0.069 ms for one proof of a 300-gate level.  UNMEASURED: every other shape, levels with long rows, the wall clock of a
 * round (which the host's opening bounds), and more than 256 proofs.  Out of scope: `_dev` forms (no bpgpu_mpc_* call has one), the pool, the host mirror, bench.py, and
 * skipping the triple of a gate whose rows are public. */
int bpgpu_witness_gate_levels(size_t n, size_t n1, size_t nchi, const uint8_t *op, const uint32_t *row_ptr, const uint32_t *kind,
                              const uint32_t *idx, uint32_t *level);
typedef struct bpgpu_mpc_witness bpgpu_mpc_witness;
int bpgpu_mpc_witness_begin(bpgpu_ctx *ctx, const bpgpu_witness *w, size_t nb, int phase, const uint8_t *v, const uint8_t *inputs,
                            const uint8_t *gadget_challenges, const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O,
                            bpgpu_mpc_witness **out);
size_t bpgpu_mpc_witness_levels_left(const bpgpu_mpc_witness *s);
size_t bpgpu_mpc_witness_level_len(const bpgpu_mpc_witness *s);
int bpgpu_mpc_witness_mask(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, const uint8_t *triples, uint8_t *masked);
int bpgpu_mpc_witness_combine(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, const uint8_t *opened);
int bpgpu_mpc_witness_finish(bpgpu_ctx *ctx, bpgpu_mpc_witness *s, uint8_t *a_L, uint8_t *a_R, uint8_t *a_O);
void bpgpu_mpc_witness_destroy(bpgpu_ctx *ctx, bpgpu_mpc_witness *s);

/* out[i] = scalars[i] * (curve generator) -- GeneratorsChain::next (generators.rs:112-124),
 * Q = w * B (prover.rs:687), PedersenGens::commit with B = B_blinding (generators.rs:41-43,61-70) */
int bpgpu_generator_mul(bpgpu_ctx *ctx, const uint8_t *scalars, size_t n, uint8_t *out);

/* Point wire codec: StarkPoint::from_bytes / to_bytes at r1cs/proof.rs:90-108,150-155 and
 * inner_product_proof.rs:391-392,440-445.  The 32-byte form lives in the absent crate mpc-stark; restated as
 * arkworks' compressed short-Weierstrass encoding: x little-endian, bit 7 of byte 31 = "y is the larger of (y, -y)",
 * bit 6 = point at infinity (parity unpinned).  Decompression takes a square root in F_p
 * (2-adicity 192) per point on the device.  ok[i] = 1 iff encoding i is valid (canonical x on the curve, not both
 * flags); invalid ones decode to 64 zero bytes -- the caller maps them to FormatError.  xy: n x 64 B boundary form. */
int bpgpu_points_decompress(bpgpu_ctx *ctx, const uint8_t *compressed, size_t n, uint8_t *xy, int32_t *ok);
/* BPGPU_E_ARG when a point is not canonical / not on the curve */
int bpgpu_points_compress(bpgpu_ctx *ctx, const uint8_t *xy, size_t n, uint8_t *compressed);

/* Batched Verifier::verify arithmetic -- r1cs/verifier.rs:457-553 for nb proofs of ONE circuit.
 * Per proof p (all arrays proof-major):
 *   points     : (11 + m + 2k) x 64 B : A_I1 A_O1 S1 A_I2 A_O2 S2 | V_0..V_{m-1} | T_1 T_3 T_4 T_5 T_6 | L_0..L_{k-1} | R_0..R_{k-1}
 *   scalars    : 5 x 32 B             : t_x t_x_blinding e_blinding a b
 *   challenges : (6 + k) x 32 B       : y z u x w r u_1..u_k   (from the host transcript, verifier.rs:432-455,506)
 * n1 = phase-1 multipliers (verifier.rs:400); padded_n = 2^k.
 * Outputs: ok[p] = 1 iff mega_check is the identity (verifier.rs:549); mega (optional, nb x 64 B) the
 * mega_check point itself; msm_scalars (optional, nb x nterms x 32 B) the scalars of verifier.rs:517-532
 * in that order, nterms = 13 + m + 2*padded_n + 2k.
 * The identity checks of transcript.rs:101-113 belong to the host transcript replay. */
int bpgpu_r1cs_verify_batch(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                            size_t n1, size_t k, const uint8_t *points, const uint8_t *scalars,
                            const uint8_t *challenges, int32_t *ok, uint8_t *mega, uint8_t *msm_scalars);
/* same with device-resident inputs/outputs (mega_dev / msm_scalars_dev may be NULL); asynchronous */
int bpgpu_r1cs_verify_batch_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                size_t n1, size_t k, const void *points_dev, const void *scalars_dev,
                                const void *challenges_dev, void *ok_dev, void *mega_dev,
                                void *msm_scalars_dev);

/* A STREAM of batches in ONE call on ONE context: the same per-proof verification for any number of proofs of one circuit.  The
 * library cuts them into batches of BPGPU_OPT_STREAM_BATCH proofs (1024) that take turns on a ring of BPGPU_OPT_STREAM_LANES (20)
 * internal streams + workspaces, so that the kernel chains of ~20 batches overlap on the GPU -- the pipelined rate (4 M
 * verifications/s for the 64-bit range gadget) without the caller creating contexts or exporting GPU_MAX_HW_QUEUES (libbpgpu.so
 * raises it to 24 when it is loaded, an inherited smaller value included; BPGPU_HW_QUEUES overrides that, 0 = hands off: see
 * bpgpu_hw_queues above.  A process that has initialised HIP before loading the library, or that sets BPGPU_HW_QUEUES=0 under an
 * inherited 4, keeps the runtime's 4 queues and a third to two thirds of the rate).  This is what a Rust host's loop of Verifier::verify
 * (verifier.rs:393) becomes: collect the proofs of one circuit, one call.
 *   _dev : operands and ok[] resident in HBM (layouts of bpgpu_r1cs_verify_batch); asynchronous -- the lanes fork from the
 *          context's stream and are joined back into it: bpgpu_sync, or the next call on this context, waits for all of them.
 *   host : operands and ok[] in host memory (page-locked from bpgpu_host_alloc for DMA speed): each batch's upload, kernels and
 *          verdict download run on its lane, so the copies of one batch overlap the kernels of the others; returns when done. */
int bpgpu_r1cs_verify_stream_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                 const void *points_dev, const void *scalars_dev, const void *challenges_dev, void *ok_dev);
int bpgpu_r1cs_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                             const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, int32_t *ok);

/* The same with the Fiat-Shamir transcript replayed ON THE DEVICE for circuits without
 * randomized constraints: instead of challenges the caller passes, per proof, the 32-byte hash-chain state it
 * holds when it would call Verifier::new (after Transcript::new(label) + any application preamble).  The
 * device performs verifier.rs:271,303,398-455,506 and inner_product_proof.rs:269-278 (keccak256, LE
 * absorption, hash_to_scalar util.rs:252-267), rejects identity points where the reference validates
 * (transcript.rs:101-113 -> ok = 0), then proceeds as bpgpu_r1cs_verify_batch.  challenges_out (optional):
 * nb x (6 + k) x 32 B, y z u x w r u_1..u_k.  The hash chain is the build's stand-in for merlin's
 * HashChainTranscript (absent from the reference tree; parity unpinned -- DESIGN.md). */
int bpgpu_r1cs_verify_batch_fs(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                               size_t k, const uint8_t *init_states, const uint8_t *points, const uint8_t *scalars,
                               int32_t *ok, uint8_t *mega, uint8_t *challenges_out);
int bpgpu_r1cs_verify_batch_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                   size_t n1, size_t k, const void *init_states_dev, const void *points_dev,
                                   const void *scalars_dev, void *ok_dev, void *mega_dev, void *challenges_out_dev);

/* The whole of Verifier::verify from the reference's WIRE format, on the device: R1CSProof::from_bytes
 * (r1cs/proof.rs:128-207: version byte, 8 or 11 compressed points, 3 big-endian scalars, k (L, R) pairs, a, b),
 * point decompression, the transcript replay and the verification of bpgpu_r1cs_verify_batch_fs, for nb proofs of
 * one circuit without randomized constraints that all have the same length (the length fixes version and k).
 * proofs: nb x proof_len B; commitments: nb x m x 32 B compressed (as a node receives them); init_states: nb x 32 B.
 * ok[p] = 1 iff proof p decodes (otherwise the reference returns FormatError) and verifies.  BPGPU_E_LEN when
 * proof_len is not a valid proof size. */
int bpgpu_r1cs_verify_batch_wire(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                 size_t proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                 const uint8_t *init_states, int32_t *ok);
int bpgpu_r1cs_verify_batch_wire_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                     size_t proof_len, const void *proofs_dev, const void *commitments_dev,
                                     const void *init_states_dev, void *ok_dev);

/* bpgpu_r1cs_verify_batch_wire for ONE two-phase circuit (bpgpu_circuit_create_param, nchi == 1): the same call with the gadget's
 * challenge label (32 bytes, zero-padded, as bpgpu_r1cs_verify_batch_fs2), so that a version-1 proof decodes, decompresses, replays
 * and verifies on the device. */
int bpgpu_r1cs_verify_batch_wire2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                  size_t proof_len, const uint8_t gadget_label[32], const uint8_t *proofs, const uint8_t *commitments,
                                  const uint8_t *init_states, int32_t *ok);
int bpgpu_r1cs_verify_batch_wire2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                      size_t proof_len, const uint8_t gadget_label[32], const void *proofs_dev,
                                      const void *commitments_dev, const void *init_states_dev, void *ok_dev);

/* Verifier::verify for nb proofs of ONE two-phase circuit (bpgpu_circuit_create_param).  _param: as bpgpu_r1cs_verify_batch with the
 * gadget challenges (nb x nchi x 32 B, in the order the gadget drew them) beside the usual 6 + k challenges.  _fs2: as
 * bpgpu_r1cs_verify_batch_fs -- the whole transcript replay on the device, including the phase separator and the gadget's
 * challenge_scalar(gadget_label) (label zero-padded to 32 bytes; verifier.rs:373-383), whose value selects the constraint weights;
 * gadget_challenges_out (optional) returns it.  A circuit with attached labels (bpgpu_circuit_set_gadget_labels) takes gadget_label ==
 * NULL and draws its nchi challenges, each under its own label (gadget_challenges_out: nb x nchi x 32); bpgpu_r1cs_verify_batch_wire2
 * likewise.  Same per-proof rejection rules as the one-phase entry points. */
int bpgpu_r1cs_verify_batch_param(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1,
                                  size_t k, const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges,
                                  const uint8_t *gadget_challenges, int32_t *ok, uint8_t *mega, uint8_t *msm_scalars);
int bpgpu_r1cs_verify_batch_fs2(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *points,
                                const uint8_t *scalars, int32_t *ok, uint8_t *mega, uint8_t *challenges_out,
                                uint8_t *gadget_challenges_out);
int bpgpu_r1cs_verify_batch_fs2_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                    const void *init_states_dev, const uint8_t gadget_label[32], const void *points_dev,
                                    const void *scalars_dev, void *ok_dev, void *mega_dev, void *challenges_out_dev,
                                    void *gadget_challenges_out_dev);
/* ONE large proof over the GPUs of a node (BASELINE configs[3], the 2^14-shuffle): every rank runs the protocol and
 * the O(n) scalar work in full, and the multi-scalar multiplications over ITS contiguous share of the terms; the ranks all-gather
 * their partial points (64 bytes each) and add them with bpgpu_points_sum -- the only exchange on the path.
 *   bpgpu_set_shard(ctx, rank, world): prover / IPP sessions opened on this context afterwards return PARTIAL sums --
 *     bpgpu_r1cs_prover_commit: A_I, A_O, S over the rank's generators (the B_blinding term on rank 0);
 *     bpgpu_ipp_round of a resident-generator session: L, R over the rank's generators (the c Q term on rank 0); the scalar
 *     vectors are folded on every rank alike; bpgpu_ipp_run_fs refuses such a session (BPGPU_E_ARG: the rounds need the exchange).
 *     world = 1 (the default) turns it off.
 *   bpgpu_r1cs_verify_shard: the rank's partial mega_check point of one proof (layouts of bpgpu_r1cs_verify_batch with nb = 1;
 *     gadget_challenges for a parametric circuit, else NULL).  The proof verifies iff the sum over the ranks is the identity.
 *     A malformed operand (off-curve or non-canonical point, non-canonical scalar / challenge) is seen only by the rank whose
 *     share holds it, and the verdict has to be collective: that rank returns BPGPU_OK with the POISON encoding in partial_xy
 *     (64 bytes 0xFF, which is not a point), so that bpgpu_points_sum over the gathered partials fails with BPGPU_E_ARG on
 *     every rank alike -- no rank is left waiting in the all-gather.  Shape errors (BPGPU_E_LEN / _GENS) are the same on all ranks. */
int bpgpu_set_shard(bpgpu_ctx *ctx, size_t rank, size_t world);
int bpgpu_r1cs_verify_shard(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t n1, size_t k, const uint8_t *points,
                            const uint8_t *scalars, const uint8_t *challenges, const uint8_t *gadget_challenges, size_t rank, size_t world,
                            uint8_t partial_xy[64]);

/* Combined batch check (NOT a reference API -- the reference verifies proof by proof; this is
 * the usual verifier-service batching and BASELINE.json's "single big MSM"): with caller-chosen random
 * weights rho (nb x 32 B, e.g. from a CSPRNG) computes  sum_p rho_p * mega_check_p  as ONE point:
 * one fixed-base MSM over the generators with scalars sum_p rho_p s_{p,g} plus one bucket-method MSM over
 * the nb*(11+m+2k) proof points (a ZERO weight drops its proof from the check: the weights must be random and non-zero; the
 * screened entry points below test for it).  All nb proofs are valid iff the point (summed over all GPUs: all-gather
 * of the 64-byte partials over RCCL, then a local add) is the identity.  Same input layout as
 * bpgpu_r1cs_verify_batch. */
int bpgpu_r1cs_verify_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                               size_t n1, size_t k, const uint8_t *points, const uint8_t *scalars,
                               const uint8_t *challenges, const uint8_t *rho, uint8_t partial_xy[64]);
int bpgpu_r1cs_verify_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                   size_t n1, size_t k, const void *points_dev, const void *scalars_dev,
                                   const void *challenges_dev, const void *rho_dev, void *partial_xy_dev);
/* SCREENED stream: per-proof accept bits at (nearly) the combined check's price when the proofs are valid -- the usual shape of
 * a verifier service.  The call cuts the proofs into batches of BPGPU_OPT_SCREEN_BATCH proofs (2560: the combined check has a long
 * kernel chain and little work per proof, so its batches are larger than the per-proof path's), runs the combined check
 * sum_p rho_p * mega_check_p of every batch first (rho: nb x 32 B of caller-chosen random non-zero weights, unpredictable to
 * the provers, as for bpgpu_r1cs_verify_combined), sets ok[p] = 1 for every proof of a batch whose point is the identity and that
 * holds no malformed input and no zero weight (a zeroed rho buffer must not accept anything), and runs the per-proof verification
 * only for the other batches, so that ok[] is what
 * bpgpu_r1cs_verify_stream returns (up to the 2^-250 chance that random weights cancel an invalid proof).  One host-side wait
 * between the two phases (68 bytes per batch are read back).  fallback_batches (optional): how many batches took the per-proof
 * path.  No reference API (the reference verifies proof by proof); built from verifier.rs:457-553. */
int bpgpu_r1cs_verify_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                               const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, int32_t *ok,
                               size_t *fallback_batches);
/* the same with operands, weights and ok[] resident in HBM; ok_dev is complete when bpgpu_sync (or the next call on the context)
 * returns -- the call itself waits once, between its two phases */
int bpgpu_r1cs_verify_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                   const void *points_dev, const void *scalars_dev, const void *challenges_dev, const void *rho_dev,
                                   void *ok_dev, size_t *fallback_batches);
/* the whole of Verifier::verify that way: the transcript replayed on the device (bpgpu_r1cs_verify_batch_fs: init_states = the
 * 32-byte chain state per proof, 1-phase circuits) per batch, then the batch's combined check, the per-proof path (again with the
 * device transcript) only for a batch that fails either; ok[] is what bpgpu_r1cs_verify_batch_fs returns */
int bpgpu_r1cs_verify_screened_fs_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb, size_t n1, size_t k,
                                      const void *init_states_dev, const void *points_dev, const void *scalars_dev, const void *rho_dev,
                                      void *ok_dev, size_t *fallback_batches);

/* MIXED queues: proofs of SEVERAL circuits in one call (NOT a reference API; a verifier service receives wallet updates, match
 * settlements, range gadgets of several widths and shuffles at once).  One group per run of proofs of one circuit; the layouts of a
 * group's operands are those of bpgpu_r1cs_verify_batch for its circuit (gadget_challenges: nb x nchi x 32 B for a circuit of
 * bpgpu_circuit_create_param, NULL otherwise; rho: nb x 32 B random non-zero weights from the caller's CSPRNG; ok: nb int32
 * verdicts of the screened calls, ignored by the combined calls).  Two groups may share a circuit handle.
 *   _combined : sum over all groups and proofs of rho_p * mega_check_p as ONE point (64 zero bytes: every proof is valid).  For one
 *               group of a one-phase circuit it is the point bpgpu_r1cs_verify_combined returns; it all-gathers the same way.  The
 *               generator halves of all proofs share ONE fixed-base MSM (the generators are a prefix chain: a group of padded n
 *               uses G_0..G_{n-1}, H_0..H_{n-1}), the proof points ONE bucket-method MSM.  A malformed operand (off-curve or
 *               non-canonical point, non-canonical scalar, challenge, gadget challenge or weight) gives the POISON encoding (64
 *               bytes 0xFF, not a point; bpgpu_points_sum rejects it) and raises the input flag; the call itself succeeds.
 *   _screened : ok[] of every group equals what bpgpu_r1cs_verify_batch (bpgpu_r1cs_verify_batch_param for a parametric circuit)
 *               returns for it, up to the 2^-250 chance that random weights cancel an invalid proof: the concatenated queue is cut
 *               into checks of at most BPGPU_OPT_SCREEN_BATCH proofs, 2^16 proof points and BPGPU_MIXED_MAX_SEGMENTS runs of one
 *               group (a check may span several groups and split one), the combined check of every one runs over the lanes of
 *               BPGPU_OPT_STREAM_LANES, and only a check whose point is not the identity, that holds a malformed operand or a zero
 *               weight takes the per-proof path, group run by group run.  fallback_batches (optional): how many checks did.
 *   _dev      : operand pointers, ok[] and partial_xy_dev in HBM; asynchronous until bpgpu_sync (the screened call waits once,
 *               between its two phases, like bpgpu_r1cs_verify_screened_dev).
 * Shape errors fail the whole call before anything is launched: BPGPU_E_LEN (k >= 32, n1 > n, padded n = 2^k not the circuit's),
 * BPGPU_E_GENS (2^k above the generators' capacity), BPGPU_E_ARG (a null pointer, gadget challenges given to a one-phase circuit or
 * missing for a parametric one, ngroups > BPGPU_MIXED_MAX_GROUPS).  ngroups == 0 or only empty groups: BPGPU_OK, the identity.
 * Device transcripts (init_states) and wire-format proofs are not taken here: challenges come from the host's transcript replay, the
 * route a Rust host already has; bpgpu_r1cs_verify_mixed_wire_* below take wire bytes. */
#define BPGPU_MIXED_MAX_GROUPS 64
#define BPGPU_MIXED_MAX_SEGMENTS 16
typedef struct bpgpu_verify_group {
  const bpgpu_circuit *circuit;        /* one-phase, or parametric (bpgpu_circuit_create_param) */
  size_t nb, n1, k;                    /* proofs in this group, phase-1 multipliers, padded_n = 2^k */
  const void *points, *scalars, *challenges;
  const void *gadget_challenges;       /* nb x nchi x 32 B for a parametric circuit, NULL otherwise */
  const void *rho;                     /* nb x 32 B random non-zero weights */
  void *ok;                            /* nb int32 verdicts (screened calls) */
} bpgpu_verify_group;
int bpgpu_r1cs_verify_mixed_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                     uint8_t partial_xy[64]);
int bpgpu_r1cs_verify_mixed_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                         void *partial_xy_dev);
int bpgpu_r1cs_verify_mixed_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                     size_t *fallback_batches);
int bpgpu_r1cs_verify_mixed_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_verify_group *groups, size_t ngroups,
                                         size_t *fallback_batches);

/* MIXED queues of WIRE-format proofs: the same two checks from what a node receives -- R1CSProof::to_bytes, compressed commitments
 * and the 32-byte transcript state per proof -- with decoding, point decompression and the Fiat-Shamir replay on the device.  A
 * group's operands are those of bpgpu_r1cs_verify_batch_wire (bpgpu_r1cs_verify_batch_wire2 with gadget_label for a parametric
 * circuit with one gadget challenge) plus the weights; proof_len fixes the version and k for the whole group.  Per check a ragged
 * front of four launches (unpack | ONE decompression over the check's points | transcript replay, a wave per run of one group |
 * fold of the reject bits) writes the operands of the mixed check above into the lane's workspace; the square-root tables and the
 * groups' transcript schedules are set up once per call.  Scalars on the wire are read modulo n.
 *   _screened : ok[] of every group equals what bpgpu_r1cs_verify_batch_wire (_wire2) returns for that group alone, up to the 2^-250
 *               weight-cancellation chance.  A proof that does not decode (wrong version byte, off-curve or non-canonical x, both
 *               flag bits set -- in a proof point or a commitment) or whose validated point is the identity gets ok[p] = 0 and sends
 *               its check to the per-proof path; neither is an error of the call.  Checks are cut and spread as for
 *               bpgpu_r1cs_verify_mixed_screened; one host-side wait, between the two phases.
 *   _combined : the point bpgpu_r1cs_verify_mixed_combined returns on the decoded operands and the device's challenges.  An
 *               undecodable proof, an identity at a validated point or a malformed weight gives the POISON encoding and raises the
 *               input flag.
 *   _dev      : every operand pointer, ok[] and partial_xy_dev in HBM; gadget_label stays a HOST pointer.
 * Shape errors, before anything is launched: BPGPU_E_LEN (proof_len is no proof size, 2^k from it is not the circuit's padded n,
 * n1 > n), BPGPU_E_GENS (2^k above the generators' capacity), BPGPU_E_ARG (a null required pointer, a parametric circuit without a
 * label or a label given to a one-phase circuit, more than one gadget challenge, ngroups > BPGPU_MIXED_MAX_GROUPS).  ngroups == 0 or
 * only empty groups: BPGPU_OK, the identity.  Two groups may share a circuit handle, with different labels or states. */
typedef struct bpgpu_wire_group {
  const bpgpu_circuit *circuit;        /* one-phase, or parametric with nchi == 1 */
  size_t nb, n1, proof_len;            /* proofs in this group, phase-1 multipliers, bytes per proof */
  const void *proofs;                  /* nb x proof_len */
  const void *commitments;             /* nb x m x 32 B compressed; may be NULL when m == 0 */
  const void *init_states;             /* nb x 32 B chain states, as bpgpu_r1cs_verify_batch_fs */
  const uint8_t *gadget_label;         /* HOST pointer, 32 bytes zero-padded, for a parametric circuit; NULL otherwise, and for a
                                          circuit with attached labels (bpgpu_circuit_set_gadget_labels) */
  const void *rho;                     /* nb x 32 B random non-zero weights */
  void *ok;                            /* nb int32 verdicts (screened calls) */
} bpgpu_wire_group;
int bpgpu_r1cs_verify_mixed_wire_screened(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                          size_t *fallback_batches);
int bpgpu_r1cs_verify_mixed_wire_screened_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                              size_t *fallback_batches);
int bpgpu_r1cs_verify_mixed_wire_combined(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                          uint8_t partial_xy[64]);
int bpgpu_r1cs_verify_mixed_wire_combined_dev(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_wire_group *groups, size_t ngroups,
                                              void *partial_xy_dev);

/* ---- pools: queues of INDEPENDENT proofs over several GPUs from ONE process ----------------------------------------------------------
 * NOT a reference API.  A pool is a set of slots; a slot is one bpgpu_ctx on one device plus one persistent host thread that selects
 * the device once and issues every HIP call of its slot.  A pool call cuts its queue into one contiguous share per slot, every
 * non-empty slot runs the single-context entry point named below on its share, on its own thread, and the caller's thread blocks until
 * every slot has finished.  The devices run their kernel chains independently: no collective is on the data path, and the only
 * exchange is the 64-byte point per slot at the end of a combined check.  A Rust verifier or prover service is one process: this is
 * what it calls instead of creating a context, tables and a circuit per device and a thread per context by hand.  ONE proof split over
 * several GPUs is a different matter and stays with bpgpu_set_shard.
 *   Slots and devices.  devices[s] is the device of slot s; a device may appear in several slots (the list {0, 0} runs two contexts
 *     and two host threads on one GPU: that is how the pool is exercised on a one-GPU machine).  Generators and circuits are built
 *     once per DISTINCT device, on the workers of those devices at the same time, and shared by the slots of that device; _get returns
 *     the handle of the slot's device, so that every single-context entry point can still be used on the borrowed context of a slot.
 *     Creation is all or nothing: what was made before a failure is released.  Parametric circuits (bpgpu_pool_circuit_create_param:
 *     the arguments of bpgpu_circuit_create_param) serve bpgpu_pool_r1cs_prove_values alone: verification of two-phase proofs has no pool
 *     form yet, so the _verify_* calls and _prove_fs refuse such a handle with BPGPU_E_ARG before any worker is woken.  A
 *     bpgpu_pool_witness is one bpgpu_witness gate program per distinct device (bpgpu_pool_witness_create: the arguments, validation and
 *     error codes of bpgpu_witness_create, all or nothing; _get(w, slot): the program of the slot's device; _destroy before the pool).
 *   bpgpu_pool_create: BPGPU_E_ARG for a null out, a null devices, nslots == 0 or nslots > BPGPU_POOL_MAX_SLOTS; BPGPU_E_DEVICE without
 *     a HIP device or for an index outside [0, bpgpu_device_count).  bpgpu_pool_destroy joins the threads; the pool's generators and
 *     circuits are destroyed BEFORE it.
 *   bpgpu_pool_ctx lends the context of a slot (NULL for a bad slot) for bpgpu_set_option, profiling, bpgpu_last_error or any other
 *     call; such calls serialise with the pool's through the context's own mutex.  bpgpu_pool_device: the slot's device, BPGPU_E_ARG for
 *     a bad slot.
 *   bpgpu_pool_set_option applies bpgpu_set_option to every slot, all or nothing: a value that one slot refuses leaves every slot as
 *     it was.
 *   bpgpu_pool_last_error: the text of the pool's last failure -- the slot, its device and that context's own text (valid until the
 *     next call on the pool).
 *   A pool serialises its calls with one mutex: for concurrency make one pool per calling thread.
 * The split.  bpgpu_pool_shares (a diagnostic that needs no device, like bpgpu_pippenger_plan; the pool calls take their split from
 *   it and from nothing else, so the split never depends on timing or data) cuts nb items into nslots contiguous shares
 *   [lo[s], lo[s + 1]): the ceil(nb / granule) granules are dealt as evenly as possible, the earlier slots taking the extra ones, so
 *   every share but the last non-empty one is a whole multiple of granule; lo[0] = 0, lo[nslots] = nb, lo is monotone, a slot may be
 *   empty.  BPGPU_E_ARG for nslots == 0, granule == 0 or a null lo (nslots + 1 entries).  The granule is slot 0's
 *   BPGPU_OPT_STREAM_BATCH for _verify_stream, its BPGPU_OPT_SCREEN_BATCH for _verify_screened and _verify_combined, and 1 for _prove_fs and
 *   _prove_values.
 * The calls.  Operands, results and layouts are those of the single-context host forms, for the whole queue (all arrays are
 *   proof-major: a share is an offset into each); what is written for a share is exactly what the single-context call writes for it.
 *   bpgpu_pool_r1cs_verify_stream    bpgpu_r1cs_verify_stream per share; slot_proofs (optional, nslots entries): the size of each share
 *   bpgpu_pool_r1cs_verify_screened  bpgpu_r1cs_verify_screened per share; fallback_batches (optional): the sum over the slots
 *   bpgpu_pool_r1cs_verify_combined  bpgpu_r1cs_verify_combined per share, then the partial points of the non-empty slots are added by
 *                                    bpgpu_points_sum on slot 0: the point that ONE bpgpu_r1cs_verify_combined over the whole queue
 *                                    returns (64 zero bytes: every proof valid).  Between processes this reduction is the all-gather of
 *                                    the partials; inside one process it is a 64-byte hand-over per slot.
 *   bpgpu_pool_r1cs_prove_fs         bpgpu_r1cs_prove_fs per share (operands and results as there, host form)
 *   bpgpu_pool_r1cs_prove_values     bpgpu_r1cs_prove_values per share, one-phase or two-phase (operands and results as there, host form:
 *                                    commitments, verdicts and proofs from the provers' values; a rejected prover's proof rows are zero
 *                                    bytes, whichever slot it fell to); the gadget label is shared by the whole queue
 *   Shape and argument errors are found before any worker is woken, with the codes of the single-context call (BPGPU_E_ARG also for
 *   handles of another pool); nb == 0 returns BPGPU_OK and touches nothing, out_xy and fallback_batches included.  When a slot fails at
 *   run time the other slots still finish -- nothing is cancelled and nothing is left running when the call returns -- and the call
 *   returns the error of the LOWEST failing slot.  A malformed proof is no error of a verification call: ok[p] = 0, as on one context.
 * Page-locked operands (UNMEASURED rule).  bpgpu_r1cs_verify_stream reads page-locked host memory in place from a kernel.  Whether a
 *   bpgpu_host_alloc buffer is mapped on EVERY device of a node has not been tried, and a device reading memory that is not mapped for
 *   it is a GPU fault; so a slot of bpgpu_pool_r1cs_verify_stream takes the in-place route only when the runtime reports the slot's own
 *   device as the owner of its share of each operand and the first and the last byte of each share lie in one allocation.  Every other
 *   slot takes the staged copies, which are correct for any host memory.  bpgpu_r1cs_verify_stream itself and bpgpu_host_alloc are
 *   unchanged. */
#define BPGPU_POOL_MAX_SLOTS 32
typedef struct bpgpu_pool bpgpu_pool;
typedef struct bpgpu_pool_gens bpgpu_pool_gens;
typedef struct bpgpu_pool_circuit bpgpu_pool_circuit;
typedef struct bpgpu_pool_witness bpgpu_pool_witness;
int bpgpu_pool_create(const int *devices, size_t nslots, bpgpu_pool **out);
void bpgpu_pool_destroy(bpgpu_pool *pool);
size_t bpgpu_pool_slots(const bpgpu_pool *pool);
int bpgpu_pool_device(const bpgpu_pool *pool, size_t slot);
bpgpu_ctx *bpgpu_pool_ctx(bpgpu_pool *pool, size_t slot);
int bpgpu_pool_set_option(bpgpu_pool *pool, int option, int64_t value);
const char *bpgpu_pool_last_error(bpgpu_pool *pool);
int bpgpu_pool_gens_create(bpgpu_pool *pool, const uint8_t *G, const uint8_t *H, size_t gens_capacity, const uint8_t B[64],
                           const uint8_t B_blinding[64], int window_bits, bpgpu_pool_gens **out);
void bpgpu_pool_gens_destroy(bpgpu_pool *pool, bpgpu_pool_gens *g);
const bpgpu_gens *bpgpu_pool_gens_get(const bpgpu_pool_gens *g, size_t slot);
int bpgpu_pool_circuit_create(bpgpu_pool *pool, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                              const uint8_t *coeff, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out);
int bpgpu_pool_circuit_create_ark(bpgpu_pool *pool, size_t q, const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx,
                                  const uint8_t *coeff_ark, size_t n_multipliers, size_t m_commitments, bpgpu_pool_circuit **out);
int bpgpu_pool_circuit_create_param(bpgpu_pool *pool, size_t q, size_t nchi, const uint32_t *row_ptr, const uint32_t *kind,
                                    const uint32_t *idx, const uint8_t *coeff, size_t n_multipliers, size_t m_commitments,
                                    bpgpu_pool_circuit **out);
/* bpgpu_circuit_set_gadget_labels on every slot's handle (for bpgpu_pool_r1cs_prove_values with gadget_label == NULL) */
int bpgpu_pool_circuit_set_gadget_labels(bpgpu_pool *pool, bpgpu_pool_circuit *c, const uint8_t *labels);
void bpgpu_pool_circuit_destroy(bpgpu_pool *pool, bpgpu_pool_circuit *c);
const bpgpu_circuit *bpgpu_pool_circuit_get(const bpgpu_pool_circuit *c, size_t slot);
int bpgpu_pool_witness_create(bpgpu_pool *pool, size_t n, size_t n1, size_t m, size_t nchi, const uint8_t *op, const uint32_t *arg,
                              const uint32_t *row_ptr, const uint32_t *kind, const uint32_t *idx, const uint8_t *coeff,
                              bpgpu_pool_witness **out);
void bpgpu_pool_witness_destroy(bpgpu_pool *pool, bpgpu_pool_witness *w);
const bpgpu_witness *bpgpu_pool_witness_get(const bpgpu_pool_witness *w, size_t slot);
int bpgpu_pool_shares(size_t nb, size_t nslots, size_t granule, size_t *lo);
int bpgpu_pool_r1cs_verify_stream(bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, size_t nb, size_t n1, size_t k,
                                  const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, int32_t *ok, size_t *slot_proofs);
int bpgpu_pool_r1cs_verify_screened(bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, size_t nb, size_t n1, size_t k,
                                    const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho, int32_t *ok,
                                    size_t *fallback_batches);
int bpgpu_pool_r1cs_verify_combined(bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, size_t nb, size_t n1, size_t k,
                                    const uint8_t *points, const uint8_t *scalars, const uint8_t *challenges, const uint8_t *rho,
                                    uint8_t out_xy[64]);
int bpgpu_pool_r1cs_prove_fs(bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, size_t nb, const uint8_t *states_in,
                             const uint8_t *a_L, const uint8_t *a_R, const uint8_t *a_O, const uint8_t *s_L, const uint8_t *s_R,
                             const uint8_t *vector_keys, const uint8_t *v_blinding, const uint8_t *blindings, uint8_t *proof_points,
                             uint8_t *proof_scalars, uint8_t *wire, uint8_t *challenges_out, uint8_t *states_out);
int bpgpu_pool_r1cs_prove_values(bpgpu_pool *pool, const bpgpu_pool_gens *g, const bpgpu_pool_circuit *c, const bpgpu_pool_witness *w,
                                 size_t nb, const uint8_t *init_states, const uint8_t gadget_label[32], const uint8_t *v,
                                 const uint8_t *v_blinding, const uint8_t *inputs, const uint8_t *s_L, const uint8_t *s_R,
                                 const uint8_t *vector_keys, const uint8_t *blindings, uint8_t *V, uint8_t *V_compressed, int32_t *ok,
                                 int64_t *first_bad_row, int64_t *first_bad_gate, uint8_t *proof_points, uint8_t *proof_scalars, uint8_t *wire,
                                 uint8_t *challenges_out, uint8_t *states_out, uint8_t *gadget_challenges_out, uint8_t *a_L_out,
                                 uint8_t *a_R_out, uint8_t *a_O_out);

#ifdef __cplusplus
}
#endif
#endif
