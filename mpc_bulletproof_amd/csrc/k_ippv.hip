// k_ippv.hip -- InnerProductProof::verify (inner_product_proof.rs:317-372) for nb proofs of one length n = 2^k: the scalar
// half (header, assembly), the operand points brought into the layout of the MSM routes, and the verdict.  The MSM itself is
// the existing routes' (bpgpu_api.hip: window-parallel / bucket method / resident-generator table walk).
//
//   expect_P = a b Q + sum_i a s_i Gf_i G_i + sum_i b s_{n-1-i} Hf_i H_i - sum_j u_j^2 L_j - sum_j u_j^-2 R_j,   ok = (expect_P == P)
//   s_i = (u_1 ... u_k)^-1 prod_{bit b of i} u^2_{k-1-b}      (closed form of the reference's induction :298-307)
//
// The vector s is never stored: an element's product over the bits of i splits into a low part (r = min(k, log2 of the block)
// bits: a table of 2^r products in LDS, built by the block) and a high part that is ONE value per block, because a block covers
// 2^r consecutive i.  s_{n-1-i} reads the same table at the complemented index.  Two multiplications per s instead of k.
#include "ec_dev.cuh"
#include "fn_dev.cuh"

using namespace bp;

namespace bpk {

// ---- header: a lane per proof.  hdr[p] = (k + 2) raw field elements: u_j^2 (j < k), a / (u_1 ... u_k), b / (u_1 ... u_k).
// Writes the scalars of Q (a b, or a b w: Q = w B), of L (-u^2) and of R (-u^-2) where the MSM route reads them.  A zero
// challenge has no inverse: the proof is marked rejected (reject[p] = 1) and computed with 1 in its place.
__global__ void __launch_bounds__(64) k_ippv_header(IppvHeader h) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= h.nb) return;
  const int k = h.k;
  bool canonical = words_canonical(&h.ab[2 * p]) && words_canonical(&h.ab[2 * p + 1]) && (!h.w || words_canonical(&h.w[p]));
  Fn pref[32], val[32];
  Fn acc = fe_one<FN>();
  bool zero = false;
#pragma unroll 1
  for (int i = 0; i < k; i++) {
    canonical = canonical && words_canonical(&h.challenges[p * k + i]);
    pref[i] = acc;
    val[i] = load_plain(&h.challenges[p * k + i]);
    if (is_zero_exact(val[i])) { zero = true; val[i] = fe_one<FN>(); }
    acc = mul(acc, val[i]);
  }
  if (!canonical) atomicOr(h.bad, 1);
  if (zero) h.reject[p] = 1;
  Fn ai = inv(acc);
  const Fn allinv = ai;
  int32_t *out = h.hdr + p * (size_t)(k + 2) * NL;
#pragma unroll 1
  for (int i = k - 1; i >= 0; i--) {
    const Fn ui = mul(ai, pref[i]);
    ai = mul(ai, val[i]);
    const Fn us = sqr(val[i]);
    raw_put(out + i * NL, us);
    store_plain(&h.l_sc[p * h.lr_stride + i], neg(us));
    store_plain(&h.r_sc[p * h.lr_stride + i], neg(sqr(ui)));
  }
  const Fn a = load_plain(&h.ab[2 * p]), b = load_plain(&h.ab[2 * p + 1]);
  raw_put(out + k * NL, mul(a, allinv));
  raw_put(out + (k + 1) * NL, mul(b, allinv));
  Fn q = mul(a, b);
  if (h.w) q = mul(q, load_plain(&h.w[p]));
  store_plain(&h.q_sc[p * h.q_stride], q);
  if (h.zero_sc) {   // resident generators: the B_blinding term
    Words8 z{};
    h.zero_sc[p * h.q_stride] = z;
  }
}
void ippv_header(hipStream_t st, const IppvHeader &h) {
  if (!h.nb) return;
  hipLaunchKernelGGL(k_ippv_header, dim3((h.nb + 63) / 64), dim3(64), 0, st, h);
}

// ---- assembly: block (proof p, chunk c) writes g_sc[p][i] = a s_i Gf_i and h_sc[p][i] = b s_{n-1-i} Hf_i for its TPB
// consecutive i.  LOG = log2(TPB); r = min(k, LOG) low bits come from the LDS table, the k - r high bits are the chunk's.
template <int LOG>
__global__ void __launch_bounds__(1 << LOG) k_ippv_assemble(size_t n, int k, size_t chunks, const int32_t *hdr, const Words8 *Gf,
                                                            const Words8 *Hf, Words8 *g_sc, Words8 *h_sc, size_t sc_stride, int *bad) {
  constexpr int TPB = 1 << LOG;
  __shared__ int32_t lo[TPB * NL];
  __shared__ int32_t hi[2 * NL];
  const size_t p = blockIdx.x / chunks, base = (blockIdx.x % chunks) * TPB;
  const int r = k < LOG ? k : LOG, t = threadIdx.x;
  const int32_t *h = hdr + p * (size_t)(k + 2) * NL;
  if (t < (1 << r)) {
    Fn v = fe_one<FN>();
    for (int b = 0; b < r; b++)
      if ((t >> b) & 1) v = mul(v, raw_get(h + (k - 1 - b) * NL));
    raw_put(lo + t * NL, v);
  }
  if (t >= TPB - 2) {   // the chunk's two high parts, with a / allinv and b / allinv folded in (the last lanes: idle in the table build of short proofs)
    const int which = t - (TPB - 2);
    const size_t idx = (which == 0 ? base : n - 1 - base) >> r;
    Fn v = raw_get(h + (k + which) * NL);
    for (int b = 0; b < k - r; b++)
      if ((idx >> b) & 1) v = mul(v, raw_get(h + (k - 1 - (r + b)) * NL));
    raw_put(hi + which * NL, v);
  }
  __syncthreads();
  const size_t i = base + t;
  if (i >= n) return;
  const size_t mask = ((size_t)1 << r) - 1;
  const Words8 *gf = &Gf[p * n + i], *hf = &Hf[p * n + i];
  if (!words_canonical(gf) || !words_canonical(hf)) atomicOr(bad, 1);
  const Fn sg = mul(raw_get(hi), raw_get(lo + (i & mask) * NL));
  const Fn sh = mul(raw_get(hi + NL), raw_get(lo + ((n - 1 - i) & mask) * NL));
  store_plain(&g_sc[p * sc_stride + i], mul(sg, load_plain(gf)));
  store_plain(&h_sc[p * sc_stride + i], mul(sh, load_plain(hf)));
}
bool ippv_assemble_fits(size_t nb, size_t n) {
  const size_t chunks = n <= 64 ? 1 : (n + 255) / 256;
  return nb <= ((size_t)1 << 31) / chunks - 1;
}
void ippv_assemble(hipStream_t st, size_t nb, size_t n, size_t k, const int32_t *hdr, const Words8 *Gf, const Words8 *Hf, Words8 *g_sc,
                   Words8 *h_sc, size_t sc_stride, int *bad) {
  if (!nb) return;
  if (n <= 64) {
    hipLaunchKernelGGL(k_ippv_assemble<6>, dim3(nb), dim3(64), 0, st, n, (int)k, (size_t)1, hdr, Gf, Hf, g_sc, h_sc, sc_stride, bad);
  } else {
    const size_t chunks = (n + 255) / 256;
    hipLaunchKernelGGL(k_ippv_assemble<8>, dim3(nb * chunks), dim3(256), 0, st, n, (int)k, chunks, hdr, Gf, Hf, g_sc, h_sc, sc_stride, bad);
  }
}

// ---- operand points: boundary bytes -> validated Montgomery affine rows, written where the MSM instance of their proof reads
// them (dense instances of `stride` rows; rows [used, stride) are padding: identity points with zero scalars).  A check_only
// segment is validated and not stored (P).  One lane per (proof, row); *bad |= 1 on a non-canonical or off-curve point.
__global__ void __launch_bounds__(256) k_ippv_points(IppvPoints a) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = a.stride + a.extra;
  if (t >= a.nb * per) return;
  const size_t p = t / per;
  size_t j = t % per;
  if (j >= a.used && j < a.stride) {   // padding
    AffDev z{};
    a.dst[p * a.stride + j] = z;
    Words8 zs{};
    a.pad_sc[p * a.stride + j] = zs;
    return;
  }
  // rows [0, used) are the segments with a destination, in order; rows [stride, stride + extra) the validate-only ones
  const bool check_only = j >= a.stride;
  size_t q = check_only ? j - a.stride : j;
  const Words8 *src = nullptr;
  for (int s = 0; s < a.nseg; s++) {
    if ((a.seg[s].check_only != 0) != check_only) continue;
    if (q < a.seg[s].cnt) { src = a.seg[s].src + 2 * (p * a.seg[s].outer + q); break; }
    q -= a.seg[s].cnt;
  }
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = src[0].w[i]; w[8 + i] = src[1].w[i]; }
  Aff pt;
  if (!aff_from_boundary(pt, w)) {
    atomicOr(a.bad, 1);
    pt.x = fe_zero<FP>();
    pt.y = fe_zero<FP>();
  }
  if (!check_only) aff_store(&a.dst[p * a.stride + j], pt);
}
void ippv_points(hipStream_t st, const IppvPoints &a) {
  const size_t tot = a.nb * (a.stride + a.extra);
  if (!tot) return;
  hipLaunchKernelGGL(k_ippv_points, dim3((tot + 255) / 256), dim3(256), 0, st, a);
}

// ---- verdict: ok[p] = (expect_P[p] == P[p]) and no reject mark.  Both are canonical boundary encodings (P validated by
// k_ippv_points, expect_P written by the MSM tail), so equal points have equal bytes.
__global__ void __launch_bounds__(256) k_ippv_verdict(size_t nb, const Words8 *expect_xy, const Words8 *P_xy, const int32_t *reject, int32_t *ok) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nb) return;
  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) diff |= (expect_xy[2 * p].w[j] ^ P_xy[2 * p].w[j]) | (expect_xy[2 * p + 1].w[j] ^ P_xy[2 * p + 1].w[j]);
  ok[p] = (diff == 0 && !reject[p]) ? 1 : 0;
}
void ippv_verdict(hipStream_t st, size_t nb, const Words8 *expect_xy, const Words8 *P_xy, const int32_t *reject, int32_t *ok) {
  if (!nb) return;
  hipLaunchKernelGGL(k_ippv_verdict, dim3((nb + 255) / 256), dim3(256), 0, st, nb, expect_xy, P_xy, reject, ok);
}

}  // namespace bpk
