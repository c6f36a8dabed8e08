// k_prove_fs.hip -- the small links between the stages of the one-call prover (bpgpu_r1cs_prove_fs: Prover::prove, r1cs/prover.rs:412-727,
// for a circuit without randomized constraints, with the transcript on the device).  The stages themselves are the staged entry
// points' kernels (phase commitments, polynomial build, fixed-base MSMs, the IPP session and its rounds) and the transcript slices
// of k_transcript.hip; here: the scalar rows of the T commitments, the scalars between the x and the w challenge, proof assembly.
// The two calls of a two-phase prover (bpgpu_r1cs_prove_fs2_begin / _finish) use the same links: the glue with the second phase's
// blinding factors and u, the assembly with a second commitment triple.
// Each launch is a short link of one batch's latency chain -- a lane per proof (or per output item), nothing to tune for throughput.
#include "fe29_sqrt.cuh"
#include "fn_dev.cuh"
#include "kernels.h"

using namespace bp;

namespace bpk {

// T_j = t_j B + tb_j B_blinding for j in {1, 3, 4, 5, 6} (prover.rs:627-631) as rows of msm_gens over [B, B_blinding] (n = 0):
// rows[(5 p + j) * 2] = (t_j, tb_j).  t: nb x 6 (t1..t6); bl: nb x 8 (i o s blinding, tb1 tb3 tb4 tb5 tb6), both plain canonical.
__global__ void __launch_bounds__(256) k_pfs_t_rows(size_t nb, const Words8 *t, const Words8 *bl, Words8 *rows) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nb * 5) return;
  const size_t p = r / 5, j = r % 5;
  rows[2 * r] = t[p * 6 + (j ? j + 1 : 0)];
  rows[2 * r + 1] = bl[p * 8 + 3 + j];
}
void prove_fs_t_rows(hipStream_t st, size_t nb, const Words8 *t, const Words8 *bl, Words8 *rows) {
  if (nb) hipLaunchKernelGGL(k_pfs_t_rows, dim3((nb * 5 + 255) / 256), dim3(256), 0, st, nb, t, bl, rows);
}

// prover.rs:644-678, a lane per proof (u = nullptr: n2 = 0, no second phase -- the u terms of :674-676 vanish):
//   tb2 = <wV, v_blinding>                       (:644-648; m <= PROVE_FS_DOT_LANE_MAX: here, a serial loop; above: tb2_pre, which
//                                                 sc_dot_batched -- a block per proof, shuffle + LDS reduction -- has computed)
//   t_x = sum_i t_i x^i, t_x_blinding = sum_i tb_i x^i  (i = 1..6, util.rs:192-194);  e_blinding = x (i_b + x (o_b + x s_b))  (:678)
//   with i_b = i1 + u i2 etc. (:674-676) for two phases: bl's first three are then i2 o2 s2, bl1 (nb x 3) holds i1 o1 s1
// out: nb x 3 (t_x, t_x_blinding, e_blinding), plain canonical -- the third transcript slice absorbs them from there.
__global__ void __launch_bounds__(64) k_pfs_glue(size_t nb, size_t m, const Words8 *x, const Words8 *t, const Words8 *bl, const Words8 *wV,
                                                 const Words8 *vb, const Words8 *tb2_pre, Words8 *out, const Words8 *u, const Words8 *bl1) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nb) return;
  Fn tb2 = fe_zero<FN>();
  if (tb2_pre) tb2 = load_plain(&tb2_pre[p]);
  else {
    for (size_t i = 0; i < m; i++) {
      tb2 = add(tb2, mul(load_plain(&wV[p * m + i]), load_plain(&vb[p * m + i])));
      if ((i & 15) == 15) tb2 = fn_reduce(tb2);
    }
    tb2 = fn_reduce(tb2);
  }
  const Fn xx = load_plain(&x[p]);
  const Words8 *tp = t + p * 6, *bp_ = bl + p * 8;
  Fn tx = load_plain(&tp[5]), tb = load_plain(&bp_[7]);
#pragma unroll 1
  for (int i = 4; i >= 0; i--) {
    tx = add(mul(tx, xx), load_plain(&tp[i]));
    // tb1 tb2 tb3 tb4 tb5 tb6: tb2 is not a draw, the others lie at bl[3], bl[4..7]
    const Fn c = i == 1 ? tb2 : load_plain(&bp_[i == 0 ? 3 : 2 + i]);
    tb = add(mul(tb, xx), c);
  }
  store_plain(&out[p * 3], mul(tx, xx));
  store_plain(&out[p * 3 + 1], mul(tb, xx));
  // the blinding factors of A_I, A_O, S: one phase: bl's first three; two (:674-676): i1 + u i2 etc., the first phase's from bl1
  Fn ib = load_plain(&bp_[0]), ob = load_plain(&bp_[1]), sb = load_plain(&bp_[2]);
  if (u) {
    const Fn uu = load_plain(&u[p]);
    ib = add(load_plain(&bl1[p * 3]), mul(uu, ib));
    ob = add(load_plain(&bl1[p * 3 + 1]), mul(uu, ob));
    sb = add(load_plain(&bl1[p * 3 + 2]), mul(uu, sb));
  }
  const Fn e = mul(xx, add(ib, mul(xx, add(ob, mul(xx, sb)))));
  store_plain(&out[p * 3 + 2], e);
}
void prove_fs_glue(hipStream_t st, size_t nb, size_t m, const Words8 *x, const Words8 *t, const Words8 *bl, const Words8 *wV, const Words8 *vb,
                   const Words8 *tb2_pre, Words8 *out, const Words8 *u, const Words8 *bl1) {
  if (nb) hipLaunchKernelGGL(k_pfs_glue, dim3((nb + 63) / 64), dim3(64), 0, st, nb, m, x, t, bl, wV, vb, tb2_pre, out, u, bl1);
}

// Proof assembly, a lane per output item of a proof: its 11 + 2k points, 5 scalars, 5 + k challenges and chain state.
//   A: nb x 3 points, T: nb x 5 points, lr: k x nb x (L, R) points (round-major, as the round loop leaves them); sc3: nb x 3 (the
//   glue's); a, b: nb; ch: 5 arrays of nb (y z u x w); uch: k arrays of nb (u_1..u_k); states: 4 x u64 per proof.
//   proof_points  nb x (11 + 2k) x 64 B : A_I1 A_O1 S1 A_I2 A_O2 S2 (identity, or A2: nb x 3 points) T_1 T_3 T_4 T_5 T_6 L_0.. R_0..
//   proof_scalars nb x 5 x 32 B        : t_x t_x_blinding e_blinding a b
//   wire (optional) nb x proof_len     : R1CSProof::to_bytes, r1cs/proof.rs:82-109 -- version byte 0, A_I1 A_O1 S1 T_1..T_6 compressed,
//                                        the three scalars big-endian, (L_j, R_j) pairs compressed, a, b big-endian; with A2: version
//                                        byte 1, A_I2 A_O2 S2 behind S1 (14 points), every later slot three further on
//   challenges_out (optional) nb x (5 + k) x 32 B : y z u x w u_1..u_k;  states_out (optional) nb x 32 B
// (ProveFsAssemble: kernels.h)
__device__ __forceinline__ void put_bytes_le(uint8_t *dst, const uint32_t w[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dst[4 * j] = (uint8_t)w[j]; dst[4 * j + 1] = (uint8_t)(w[j] >> 8); dst[4 * j + 2] = (uint8_t)(w[j] >> 16); dst[4 * j + 3] = (uint8_t)(w[j] >> 24);
  }
}
__device__ __forceinline__ void put_bytes_be(uint8_t *dst, const uint32_t w[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint8_t *d = dst + 28 - 4 * j;
    d[3] = (uint8_t)w[j]; d[2] = (uint8_t)(w[j] >> 8); d[1] = (uint8_t)(w[j] >> 16); d[0] = (uint8_t)(w[j] >> 24);
  }
}
__global__ void __launch_bounds__(256) k_pfs_assemble(ProveFsAssemble o) {
  // sh: the wire slots that A_I2 A_O2 S2 take when there is a second phase (version 1 carries all 14 points)
  const size_t k = o.k, nvar = 11 + 2 * k, per = nvar + 5 + (5 + k) + 1, sh = o.A2 ? 3 : 0, proof_len = 1 + (11 + sh) * 32 + (2 * k + 2) * 32;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= o.nb * per) return;
  const size_t p = t / per, s = t - p * per;
  uint8_t *wire = o.wire ? o.wire + p * proof_len : nullptr;
  if (s < nvar) {
    const Words8 *src = nullptr;     // identity: A_I2 A_O2 S2 of a one-phase proof
    size_t wslot = (size_t)-1;       // 32-byte slot of the wire body, none for the identity points (version 0 omits them)
    if (s < 3) { src = o.A + (p * 3 + s) * 2; wslot = s; }
    else if (s < 6) { if (o.A2) { src = o.A2 + (p * 3 + (s - 3)) * 2; wslot = s; } }
    else if (s < 11) { src = o.T + (p * 5 + (s - 6)) * 2; wslot = s - 3 + sh; }
    else if (s < 11 + k) { src = o.lr + ((s - 11) * o.nb + p) * 4; wslot = 11 + sh + 2 * (s - 11); }
    else { src = o.lr + ((s - 11 - k) * o.nb + p) * 4 + 2; wslot = 11 + sh + 2 * (s - 11 - k) + 1; }
    uint32_t x[8], y[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { x[j] = src ? src[0].w[j] : 0u; y[j] = src ? src[1].w[j] : 0u; }
    Words8 *dst = o.proof_points + (p * nvar + s) * 2;
#pragma unroll
    for (int j = 0; j < 8; j++) { dst[0].w[j] = x[j]; dst[1].w[j] = y[j]; }
    if (wire && wslot != (size_t)-1) {
      compress_xy_words(x, y);
      put_bytes_le(wire + 1 + 32 * wslot, x);
    }
    if (wire && s == 0) wire[0] = o.A2 ? 1 : 0;   // TWO_PHASE_COMMITMENTS : ONE_PHASE_COMMITMENTS
  } else if (s < nvar + 5) {
    const size_t q = s - nvar;
    const Words8 *src = q < 3 ? o.sc3 + p * 3 + q : (q == 3 ? o.a + p : o.b + p);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = src->w[j];
#pragma unroll
    for (int j = 0; j < 8; j++) o.proof_scalars[p * 5 + q].w[j] = w[j];
    if (wire) put_bytes_be(wire + 1 + 32 * (sh + (q < 3 ? 8 + q : 11 + 2 * k + (q - 3))), w);
  } else if (s < nvar + 5 + 5 + k) {
    if (!o.challenges_out) return;
    const size_t c = s - nvar - 5;
    o.challenges_out[p * (5 + k) + c] = c < 5 ? o.ch[c * o.nb + p] : o.uch[(c - 5) * o.nb + p];
  } else if (o.states_out) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint64_t v = o.states[p * 4 + i];
      o.states_out[p].w[2 * i] = (uint32_t)v; o.states_out[p].w[2 * i + 1] = (uint32_t)(v >> 32);
    }
  }
}
void prove_fs_assemble(hipStream_t st, const ProveFsAssemble &a) {
  if (!a.nb) return;
  const size_t tot = a.nb * (11 + 2 * a.k + 5 + 5 + a.k + 1);
  hipLaunchKernelGGL(k_pfs_assemble, dim3((tot + 255) / 256), dim3(256), 0, st, a);
}

// bpgpu_r1cs_prove_values: a prover whose witness failed the check (ok[p] == 0) ships nothing -- its rows of proof_points,
// proof_scalars, wire, challenges_out and states_out become zero bytes; an accepted prover's rows are not touched.  A thread per 16
// bytes of a prover's rows (per * nb threads; every store lies inside row p < nb of its array).  The wire rows are of odd length and
// start at any byte: those are cleared bytewise.
__global__ void __launch_bounds__(256) k_pfs_clear_rejected(ProveFsClear o) {
  const size_t c_pts = o.b_points / 16, c_sc = c_pts + 10, c_ch = c_sc + (o.challenges_out ? o.b_chal / 16 : 0),
               c_st = c_ch + (o.states_out ? 2 : 0), per = c_st + (o.wire ? (o.b_wire + 15) / 16 : 0);
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= o.nb * per) return;
  const size_t p = t / per, s = t - p * per;
  if (o.ok[p] != 0) return;
  if (s >= c_st) {
    const size_t lo = (s - c_st) * 16, hi = lo + 16 < o.b_wire ? lo + 16 : o.b_wire;
    uint8_t *row = o.wire + p * o.b_wire;
    for (size_t i = lo; i < hi; i++) row[i] = 0;
    return;
  }
  uint32_t *dst;
  if (s < c_pts) dst = (uint32_t *)(o.proof_points + p * o.b_points) + 4 * s;
  else if (s < c_sc) dst = (uint32_t *)(o.proof_scalars + p * 160) + 4 * (s - c_pts);
  else if (s < c_ch) dst = (uint32_t *)(o.challenges_out + p * o.b_chal) + 4 * (s - c_sc);
  else dst = (uint32_t *)(o.states_out + p * 32) + 4 * (s - c_ch);
  dst[0] = 0u; dst[1] = 0u; dst[2] = 0u; dst[3] = 0u;
}
void prove_fs_clear_rejected(hipStream_t st, const ProveFsClear &a) {
  if (!a.nb) return;
  const size_t per = a.b_points / 16 + 10 + (a.challenges_out ? a.b_chal / 16 : 0) + (a.states_out ? 2 : 0) + (a.wire ? (a.b_wire + 15) / 16 : 0);
  hipLaunchKernelGGL(k_pfs_clear_rejected, dim3((a.nb * per + 255) / 256), dim3(256), 0, st, a);
}

}  // namespace bpk
