// ec_chain.cuh -- the Horner chain over partial sums, stated once for the three arithmetic forms (ec29.cuh: a lane per chain;
// ec29_quad.cuh: a DPP quad; ec29_row.cuh: a wave).  A form type maps (block, thread) to the chain ("unit") it works on and
// names the operations of its arithmetic; horner_sum is the loop, horner_chain the loop over the chains of a launch.
// Its users: the two Horner stages of the verification (k_ec.hip), the tails of the bucket-method MSMs (k_pip.hip,
// k_pip2.hip).  ChainForm and the two helpers below it are host code, for the launchers; the rest is device code.
#pragma once
#include "ec_dev.cuh"
#include "ec29_quad.cuh"
#include "ec29_row.cuh"

namespace bpk {

enum class ChainForm : int { Lane = 0, Quad = 1, Row = 2 };
// a form option of the ABI (BPGPU_OPT_HORNER_FORM, BPGPU_OPT_GROUPS_FORM): 1 = lane, 2 = quad, 3 = row; anything else = `other`
inline ChainForm chain_form_option(int opt, ChainForm other) {
  return opt == 1 ? ChainForm::Lane : (opt == 2 ? ChainForm::Quad : (opt == 3 ? ChainForm::Row : other));
}
// blocks of 64 threads for `units` chains
inline unsigned chain_blocks(ChainForm form, size_t units) {
  return (unsigned)(form == ChainForm::Row ? units : (form == ChainForm::Quad ? (units + 15) / 16 : (units + 63) / 64));
}

// Each form: unit = the chain of this thread, active = whether the thread takes part at all, and
// first (the top partial sum, which becomes the accumulator), addend, dbl, add, store.
struct LaneForm {   // 64 chains per block; lanes past the last chain leave
  typedef Jac Pt;
  size_t unit;
  bool active;
  __device__ __forceinline__ LaneForm(size_t blk, size_t units) : unit(blk * 64 + threadIdx.x) { active = unit < units; }
  __device__ __forceinline__ Pt first(const JacRaw *s) const { return raw_load(s); }
  __device__ __forceinline__ Pt addend(const JacRaw *s) const { return raw_load(s); }
  __device__ __forceinline__ Pt dbl(const Pt &a) const { return jac_dbl(a); }
  __device__ __forceinline__ Pt add(const Pt &a, const Pt &b) const { return jac_add(a, b); }
  __device__ __forceinline__ void store(JacRaw *d, const Pt &a) const { raw_store(d, a); }
};
struct QuadForm {   // a chain per quad.  The DPP moves of q4_* need whole quads: a quad past the last chain stays active on
  typedef JacT Pt;  // a clamped index -- it recomputes the last chain -- and only live quads store.  (units >= 1: no launcher
                    // starts a grid for no chain)
  size_t unit;
  int role;
  bool live;
  static constexpr bool active = true;
  __device__ __forceinline__ QuadForm(size_t blk, size_t units) : unit((blk * blockDim.x + threadIdx.x) >> 2), role(threadIdx.x & 3) {
    live = unit < units;
    if (!live) unit = units - 1;
  }
  __device__ __forceinline__ Pt first(const JacRaw *s) const { return jact_from_jac(raw_load(s)); }
  __device__ __forceinline__ Pt addend(const JacRaw *s) const { return jact_from_jac(raw_load(s)); }
  __device__ __forceinline__ Pt dbl(const Pt &a) const { return q4_dbl(a, role); }
  __device__ __forceinline__ Pt add(const Pt &a, const Pt &b) const { return q4_add(a, b, role); }
  __device__ __forceinline__ void store(JacRaw *d, const Pt &a) const { if (live && role == 0) raw_store(d, jact_to_jac(a)); }
};
struct RowForm {    // one chain per block: the grid is the number of chains
  typedef JacR Pt;
  RowK K;
  size_t unit;
  static constexpr bool active = true;
  __device__ __forceinline__ RowForm(size_t blk, size_t /* units */) : K(rowk_init()), unit(blk) {}
  __device__ __forceinline__ Pt first(const JacRaw *s) const { return jacr_from_limbs(K, s->v); }
  // an addend carries no Th: only doublings read Th, and radd rebuilds it where the accumulator was the identity.  So an
  // addend is always the SECOND operand of add, and never becomes the accumulator by any other way
  __device__ __forceinline__ Pt addend(const JacRaw *s) const { return jacr_addend_from_limbs(K, s->v); }
  __device__ __forceinline__ Pt dbl(const Pt &a) const { return rdbl(K, a); }
  __device__ __forceinline__ Pt add(const Pt &a, const Pt &b) const { return radd(K, a, b); }
  __device__ __forceinline__ void store(JacRaw *d, const Pt &a) const { jacr_store(K, d->v, a); }
};

// sum_{w < count} 2^(dbl w) src[at + w stride]:  acc = the top term; then, downwards, `dbl` doublings and the next term.
// The chain's place in an array is an index, `at`: the callers share src and do not fold their chain's offset into it.
template <class F> __device__ __forceinline__
typename F::Pt horner_sum(const F &f, const JacRaw *src, int count, int stride, int dbl, size_t at = 0) {
  typename F::Pt acc = f.first(&src[at + (size_t)(count - 1) * stride]);
#pragma unroll 1
  for (int w = count - 2; w >= 0; w--) {
#pragma unroll 1
    for (int d = 0; d < dbl; d++) acc = f.dbl(acc);
    acc = f.add(acc, f.addend(&src[at + (size_t)w * stride]));
  }
  return acc;
}
// The chains of a launch, in form F: chain u is the sum over src[u src_pitch + w stride], stored to dst[u dst_pitch].  That
// may be the slot of the chain's last term, src[u src_pitch] (the first stage of the verification works in place): the store
// comes after every load of that slot in the storing thread, and the clamped quads that load the same slot (QuadForm) run
// in the storing quad's wave, in lockstep with it.
template <class F> __device__ __forceinline__
void horner_chain(size_t blk, size_t units, const JacRaw *src, size_t src_pitch, int count, int stride, int dbl, JacRaw *dst, size_t dst_pitch) {
  const F f(blk, units);
  if (!f.active) return;
  const typename F::Pt sum = horner_sum(f, src, count, stride, dbl, f.unit * src_pitch);
  f.store(&dst[f.unit * dst_pitch], sum);
}

}  // namespace bpk
