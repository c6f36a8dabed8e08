// ec_dev.cuh -- device helpers shared by the elliptic-curve translation units.
#pragma once
#include "ec29.cuh"
#include "kernels.h"

namespace bpk {
using namespace bp;

__device__ __forceinline__ void raw_store(JacRaw *d, const Jac &p) {
#pragma unroll
  for (int j = 0; j < NL; j++) { d->v[j] = p.X.v[j]; d->v[NL + j] = p.Y.v[j]; d->v[2 * NL + j] = p.Z.v[j]; }
}
__device__ __forceinline__ Jac raw_load(const JacRaw *s) {
  Jac p;
#pragma unroll
  for (int j = 0; j < NL; j++) { p.X.v[j] = s->v[j]; p.Y.v[j] = s->v[NL + j]; p.Z.v[j] = s->v[2 * NL + j]; }
  return p;
}
__device__ __forceinline__ Aff aff_load(const AffDev *s) {
  Aff a;
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = s->w[j];
  a.x = unpack<FP>(w);
  a.y = unpack<FP>(w + 8);
  return a;
}
__device__ __forceinline__ void aff_store(AffDev *d, const Aff &a) {
  uint32_t w[16];
  pack(w, canon(a.x));
  pack(w + 8, canon(a.y));
#pragma unroll
  for (int j = 0; j < 16; j++) d->w[j] = w[j];
}

// a boundary point (x || y, 16 words) lies in two consecutive Words8: point i of `xy` is xy[2 i], xy[2 i + 1]
__device__ __forceinline__ void boundary_load(uint32_t *w, const Words8 *xy, size_t i) {
#pragma unroll
  for (int j = 0; j < 8; j++) { w[j] = xy[2 * i].w[j]; w[8 + j] = xy[2 * i + 1].w[j]; }
}
__device__ __forceinline__ void boundary_store(Words8 *xy, size_t i, const uint32_t *w) {
#pragma unroll
  for (int j = 0; j < 8; j++) { xy[2 * i].w[j] = w[j]; xy[2 * i + 1].w[j] = w[8 + j]; }
}
// point i of `xy` = p as boundary bytes; a sum that came out with Z = 0 (mod p) in a non-zero representation is the identity
__device__ __forceinline__ void jac_store_boundary(Words8 *xy, size_t i, Jac p) {
  if (!jac_is_inf(p) && is_zero_exact(p.Z)) p = jac_inf();
  uint32_t w[16];
  aff_to_boundary(w, jac_to_aff(p));
  boundary_store(xy, i, w);
}
// the end of a verification: proof p holds if its check point `acc` is the identity and none of its inputs was malformed;
// mega (optional): the check point's boundary bytes, zeros for the identity
__device__ __forceinline__ void verdict_store(const Jac &acc, int malformed, int32_t *ok, Words8 *mega, size_t p) {
  const bool inf = jac_is_inf(acc) || is_zero_exact(acc.Z);
  ok[p] = (inf && !malformed) ? 1 : 0;
  if (mega) {
    uint32_t w[16];
    if (inf) {
#pragma unroll
      for (int j = 0; j < 16; j++) w[j] = 0;
    } else {
      aff_to_boundary(w, jac_to_aff(acc));
    }
    boundary_store(mega, p, w);
  }
}

// the point held by lane (this lane ^ off): one step of a butterfly sum is  acc = jac_add(acc, jac_shfl_xor(acc, off))
__device__ __forceinline__ Jac jac_shfl_xor(const Jac &a, int off) {
  Jac q;
#pragma unroll
  for (int t = 0; t < NL; t++) {
    q.X.v[t] = __shfl_xor(a.X.v[t], off, 64);
    q.Y.v[t] = __shfl_xor(a.Y.v[t], off, 64);
    q.Z.v[t] = __shfl_xor(a.Z.v[t], off, 64);
  }
  return q;
}

// ------------------------------------------------------------------------------------------------
// block-level point sum: every lane holds `acc`; result valid in lane 0.  smem: 27 * TPB/2 ints.
template <int TPB> __device__ __forceinline__ Jac block_sum(Jac acc, int32_t *smem) {
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (tid >= s && tid < 2 * s) {
#pragma unroll
      for (int t = 0; t < NL; t++) {
        smem[t * (TPB / 2) + tid - s] = acc.X.v[t];
        smem[(NL + t) * (TPB / 2) + tid - s] = acc.Y.v[t];
        smem[(2 * NL + t) * (TPB / 2) + tid - s] = acc.Z.v[t];
      }
    }
    __syncthreads();
    if (tid < s) {
      Jac q;
#pragma unroll
      for (int t = 0; t < NL; t++) {
        q.X.v[t] = smem[t * (TPB / 2) + tid];
        q.Y.v[t] = smem[(NL + t) * (TPB / 2) + tid];
        q.Z.v[t] = smem[(2 * NL + t) * (TPB / 2) + tid];
      }
      acc = jac_add(acc, q);
    }
    __syncthreads();
  }
  return acc;
}

}  // namespace bpk
