// k_mpc.hip -- one party's local arithmetic of the two-party (SPDZ-style) R1CS prover, src/r1cs_mpc/ of the reference.
//
// An authenticated scalar held by party p is three planes -- share s_p, MAC share m_p, public modifier c (identical at both
// parties) -- with value s_0 + s_1 + c and m_0 + m_1 = alpha (s_0 + s_1) (include/bpgpu.h).  A session of nb proofs is run as
// 3 nb "virtual provers" v = 3 p + k (k = 0 share, 1 MAC, 2 modifier): every LINEAR step is the single-party kernel over them
// (commitment rows, fixed-base walks, k_ipp_gens_scalars, the folds).  The kernels here are the steps that are not linear in one
// plane: public terms go to the modifier plane only, and a product of two shared values goes through a Beaver triple
// (x, y, z = x y) whose opened differences d = a - x, e = b - y give the product's planes z_k + d y_k + e x_k (+ d e on k = 2).
//
// Layouts (plain canonical words on the device; the API converts from / to ark-ff Montgomery form around them):
//   triples [p][j][t = x, y, z][k][i]      masked [p][j][d, e][k][i]      opened [p][j][d, e][i]
// with j the product of the step (6 in the polynomial build, 2 -- c_L, c_R -- in an IPP round) and i < len.
#include "mpc_witness_dev.cuh"   // beaver_term: the Beaver combine, stated once

using namespace bp;

namespace bpk {

// r1cs_mpc/mpc_prover.rs:783-829: the l(x) / r(x) coefficient vectors per plane, layout [6][3 nb][n][9] as k_prover_polys
// (l1 l2 l3 r0 r1 r3).  Public terms -- y^-i wR in l1, wL in r1 -- land on the modifier plane only; r0 = wO - y^i is PUBLIC and
// is stored as its value on every plane (it multiplies the shared l1, l2, l3 locally; the evaluation adds it on k = 2 only).
// The same pass writes the masked values of the six shared x shared products l1 r1, l2 r1, l3 r1, l1 r3, l2 r3, l3 r3.
__global__ void __launch_bounds__(128) k_mpc_polys(CircuitDev c, size_t nb, const Words8 *y, const Words8 *y_inv, const Words8 *a_L,
                                                   const Words8 *a_R, const Words8 *a_O, const Words8 *s_L, const Words8 *s_R,
                                                   const int32_t *zpow_all, int32_t *polys, Words8 *wV_out, const Words8 *trip,
                                                   Words8 *masked) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y, p = v / 3;
  const int k = (int)(v % 3);
  const size_t n = c.n;
  const int32_t *zp = zpow_all + p * c.qz * NL;
  if (k == 2 && i < c.m) store_plain(&wV_out[p * c.m + i], flatten_column(c, 3 * n + i, zp));
  if (i >= n) return;
  const Fn yi = fn_pow_u32(load_plain(&y[v]), (uint32_t)i);
  const Fn wO = flatten_column(c, 2 * n + i, zp);
  const size_t e = v * n + i, plane = 3 * nb * n * NL;
  Fn l1 = load_plain(&a_L[e]), r1 = mul(yi, load_plain(&a_R[e]));
  if (k == 2) {
    const Fn yni = fn_pow_u32(load_plain(&y_inv[v]), (uint32_t)i);
    l1 = add(l1, mul(yni, flatten_column(c, n + i, zp)));
    r1 = add(r1, flatten_column(c, i, zp));
  }
  const Fn l2 = load_plain(&a_O[e]), l3 = load_plain(&s_L[e]), r0 = sub(wO, yi), r3 = mul(yi, load_plain(&s_R[e]));
  int32_t *dst = polys + e * NL;
  raw_put(dst + 0 * plane, l1);
  raw_put(dst + 1 * plane, l2);
  raw_put(dst + 2 * plane, l3);
  raw_put(dst + 3 * plane, r0);
  raw_put(dst + 4 * plane, r1);
  raw_put(dst + 5 * plane, r3);
  const Fn L[3] = {l1, l2, l3};
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const Words8 *t = trip + ((p * 6 + j) * 9 + k) * n + i;
    Words8 *m = masked + ((p * 6 + j) * 6 + k) * n + i;      // d at m, e at m + 3 n
    store_plain(m, sub(L[j % 3], load_plain(t)));
    store_plain(m + 3 * n, sub(j < 3 ? r1 : r3, load_plain(t + 3 * n)));
  }
}
void mpc_polys(hipStream_t st, const CircuitDev &c, size_t nb, const Words8 *y, const Words8 *y_inv, const Words8 *a_L,
               const Words8 *a_R, const Words8 *a_O, const Words8 *s_L, const Words8 *s_R, const int32_t *zpow, int32_t *polys,
               Words8 *wV_out, const Words8 *trip, Words8 *masked) {
  const size_t span = c.n > c.m ? c.n : c.m;
  if (!nb || !span) return;
  hipLaunchKernelGGL(k_mpc_polys, dim3((span + 127) / 128, 3 * nb), dim3(128), 0, st, c, nb, y, y_inv, a_L, a_R, a_O, s_L, s_R, zpow,
                     polys, wV_out, trip, masked);
}

// t_1..t_6 per plane (util.rs:152-170 special_inner_product on shares, authenticated_poly.rs:143-164): one block per (virtual
// prover, coefficient).  The products with the public r0 are local; the six shared x shared ones come from the Beaver combine:
// t1 = <l1,r0>; t2 = P0 + <l2,r0>; t3 = P1 + <l3,r0>; t4 = P3 + P2; t5 = P4; t6 = P5.
__global__ void __launch_bounds__(256) k_mpc_tcoeffs(size_t nb, size_t n, const int32_t *polys, const Words8 *opened, const Words8 *trip,
                                                     Words8 *t_out) {
  const size_t v = blockIdx.x, p = v / 3, plane = 3 * nb * n * NL;
  const int k = (int)(v % 3), which = blockIdx.y;
  const int A[6] = {0, 1, 2, -1, -1, -1}, P1[6] = {-1, 0, 1, 3, 4, 5}, P2[6] = {-1, -1, -1, 2, -1, -1};
  const int a = A[which], p1 = P1[which], p2 = P2[which];
  Fn acc = fe_zero<FN>();
  int cnt = 0;
  for (size_t i = threadIdx.x; i < n; i += 256) {
    if (a >= 0) {
      const int32_t *e = polys + (v * n + i) * NL;
      acc = add(acc, mul(raw_get(e + a * plane), raw_get(e + 3 * plane)));
    }
    if (p1 >= 0) acc = add(acc, beaver_term(opened, trip, p, 6, (size_t)p1, k, n, i));
    if (p2 >= 0) acc = add(acc, beaver_term(opened, trip, p, 6, (size_t)p2, k, n, i));
    if ((++cnt & 3) == 0) acc = fn_reduce(acc);
  }
  const Fn t = block_sum<256>(acc);
  if (threadIdx.x == 0) store_plain(&t_out[v * 6 + which], t);
}
void mpc_tcoeffs(hipStream_t st, size_t nb, size_t n, const int32_t *polys, const Words8 *opened, const Words8 *trip, Words8 *t_out) {
  if (!nb) return;
  hipLaunchKernelGGL(k_mpc_tcoeffs, dim3(3 * nb, 6), dim3(256), 0, st, nb, n, polys, opened, trip, t_out);
}

// scalar rows of the T commitments, T_j = t_j B + tb_j B_blinding per plane (mpc_prover.rs:836-856 commit_shared): MSM 5 v + j over
// [B, B_blinding] for j = T_1, T_3, T_4, T_5, T_6
__global__ void __launch_bounds__(256) k_mpc_t_rows(size_t nvirt, const Words8 *t, const Words8 *tb, Words8 *rows) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nvirt * 5) return;
  const size_t v = r / 5, j = r % 5;
  rows[2 * r] = t[v * 6 + (j ? j + 1 : 0)];
  rows[2 * r + 1] = tb[r];
}
void mpc_t_rows(hipStream_t st, size_t nvirt, const Words8 *t, const Words8 *tb, Words8 *rows) {
  if (!nvirt) return;
  hipLaunchKernelGGL(k_mpc_t_rows, dim3((nvirt * 5 + 255) / 256), dim3(256), 0, st, nvirt, t, tb, rows);
}

// mpc_prover.rs:901-917: l(x), r(x) per plane; the public r0 and the -y^i padding of r on the modifier plane only
__global__ void __launch_bounds__(128) k_mpc_eval(size_t nb, size_t n, size_t np, const Words8 *x, const Words8 *y, const int32_t *polys,
                                                  Words8 *l_vec, Words8 *r_vec) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y;
  if (i >= np) return;
  const bool mod = v % 3 == 2;
  if (i < n) {
    const Fn xx = load_plain(&x[v]);
    const size_t plane = 3 * nb * n * NL;
    const int32_t *e = polys + (v * n + i) * NL;
    const Fn l = mul(xx, add(raw_get(e), mul(xx, add(raw_get(e + plane), mul(xx, raw_get(e + 2 * plane))))));
    Fn r = mul(xx, add(raw_get(e + 4 * plane), mul(xx, mul(xx, raw_get(e + 5 * plane)))));
    if (mod) r = add(r, raw_get(e + 3 * plane));
    store_plain(&l_vec[v * np + i], l);
    store_plain(&r_vec[v * np + i], r);
  } else {
    store_plain(&l_vec[v * np + i], fe_zero<FN>());
    store_plain(&r_vec[v * np + i], mod ? neg(fn_pow_u32(load_plain(&y[v]), (uint32_t)i)) : fe_zero<FN>());
  }
}
void mpc_eval(hipStream_t st, size_t nb, size_t n, size_t padded_n, const Words8 *x, const Words8 *y, const int32_t *polys, Words8 *l_vec,
              Words8 *r_vec) {
  if (!nb || !padded_n) return;
  hipLaunchKernelGGL(k_mpc_eval, dim3((padded_n + 127) / 128, 3 * nb), dim3(128), 0, st, nb, n, padded_n, x, y, polys, l_vec, r_vec);
}

// mpc_inner_product.rs:142-155 (first round) / :202-215: masked values of c_L = <a_L, b_R> (j = 0) and c_R = <a_R, b_L> (j = 1)
// for the session's current vectors a, b (3 nb x 2h)
__global__ void __launch_bounds__(256) k_mpc_ipp_mask(size_t h, const Words8 *a, const Words8 *b, const Words8 *trip, Words8 *masked) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y, p = v / 3;
  if (i >= h) return;
  const int k = (int)(v % 3);
  const Words8 *ap = a + v * 2 * h, *bp = b + v * 2 * h;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const Words8 *t = trip + ((p * 2 + j) * 9 + k) * h + i;
    Words8 *m = masked + ((p * 2 + j) * 6 + k) * h + i;
    store_plain(m, sub(load_plain(&ap[j ? h + i : i]), load_plain(t)));
    store_plain(m + 3 * h, sub(load_plain(&bp[j ? i : h + i]), load_plain(t + 3 * h)));
  }
}
void mpc_ipp_mask(hipStream_t st, size_t nb, size_t h, const Words8 *a, const Words8 *b, const Words8 *trip, Words8 *masked) {
  if (!nb || !h) return;
  hipLaunchKernelGGL(k_mpc_ipp_mask, dim3((h + 255) / 256, 3 * nb), dim3(256), 0, st, h, a, b, trip, masked);
}
// the Beaver combine of c_L, c_R reduced per (virtual prover, product) into the session's cLR (2 per virtual prover), which the
// round's k_ipp_gens_scalars then reads as the single-party round reads sc_dot_batched's
__global__ void __launch_bounds__(256) k_mpc_ipp_combine(size_t h, const Words8 *opened, const Words8 *trip, Words8 *cLR) {
  const size_t v = blockIdx.x, p = v / 3, j = blockIdx.y;
  const int k = (int)(v % 3);
  Fn acc = fe_zero<FN>();
  int cnt = 0;
  for (size_t i = threadIdx.x; i < h; i += 256) {
    acc = add(acc, beaver_term(opened, trip, p, 2, j, k, h, i));
    if ((++cnt & 7) == 0) acc = fn_reduce(acc);
  }
  const Fn t = block_sum<256>(acc);
  if (threadIdx.x == 0) store_plain(&cLR[2 * v + j], t);
}
void mpc_ipp_combine(hipStream_t st, size_t nb, size_t h, const Words8 *opened, const Words8 *trip, Words8 *cLR) {
  if (!nb) return;
  hipLaunchKernelGGL(k_mpc_ipp_combine, dim3(3 * nb, 2), dim3(256), 0, st, h, opened, trip, cLR);
}

}  // namespace bpk
