// k_witness.hip -- witness synthesis: the gates of a bpgpu_witness program (Prover::multiply, prover.rs:99-125; allocate_multiplier,
// :148-165) for nb provers, one launch per phase, in three forms.  The gate itself is wit_gate_values of witness_dev.cuh; the rows are
// eval_row's (fn_dev.cuh).  The planes a launch works on are the library's own scratch, plain canonical words: witness_convert takes
// the callers' ark planes in and out, prover by prover, so that a phase can land in planes of its own stride.
#include "fe29_consts.h"
#include "witness_scan.cuh"

using namespace bp;

namespace bpk {

struct WitArgs {
  WitDev w;
  size_t nb;
  uint32_t g_lo, g_hi, l_lo, l_hi;
  Words8 *aL, *aR, *aO;
  const Words8 *v, *inputs, *chi;
};
// what one prover reads and writes (chi: never read when no term has j > 0, as in eval_row)
struct WitProver { Words8 *aL, *aR, *aO; const Words8 *v, *inputs, *chi; };
__device__ __forceinline__ WitProver wit_prover(const WitArgs &a, size_t p) {
  return {a.aL + p * a.w.n, a.aR + p * a.w.n, a.aO + p * a.w.n, a.v + p * a.w.m, a.inputs + p * a.w.ninp * 2, a.chi + p * a.w.nchi};
}

// A lane per prover: the gates in program order, which is topological (a term reads a gate below its own), so a lane only ever
// reads what it has stored itself.
// The three kernels are templated on INV, whether the launch's range holds an INV gate: the <.., false> instantiations are the
// kernels of a program without one, with no inversion in them and no read of level_inv / scan_inv.  DIV is the same for a DIVREM
// gate (int_div.cuh): the <.., false> instantiations carry no integer division.  A DIVREM gate is an ordinary gate of its level --
// strided over the threads with the others, nothing to batch -- and with a long row lane 0 divides.
template <bool INV, bool DIV> __global__ void __launch_bounds__(256) k_witness_lane(WitArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.nb) return;
  const WitProver o = wit_prover(a, p);
  for (uint32_t i = a.g_lo; i < a.g_hi; i++) wit_gate_lane_of<INV, DIV>(a.w, i, o.aL, o.aR, o.aO, o.v, o.inputs, o.chi);
}
// A block per prover: level by level.  The gates of a level read lower levels only (or earlier phases), so they are independent:
// those without a long row are strided over the 256 threads, the others over the four waves (lane-strided terms, then wave_sum, as
// k_rows_eval does).  Between two levels the plane stores of the one are made visible to the block (they are global stores that
// other waves of this block load: a block-scope fence, then the barrier).  Every thread of the block reaches every barrier: the
// level range is the launch's, and no thread leaves early.  wit_level_gates: the gates order[lo .. mid) (short rows) and
// order[mid .. hi) (a long row) of one level.  With INV, the short-row INV gates are order[inv .. mid), strided over the threads
// like the others, and a thread inverts ONCE per level for all of its own (witness_dev.cuh wit_inv_forward / _backward): it reads
// back only what it parked itself, so the level needs no fence or barrier of its own; the loop bounds are block-uniform, and a
// thread without an INV gate inverts 1.  Without INV, inv == mid.  An INV gate with a long row is lane 0's, one inversion each.
template <bool INV, bool DIV>
__device__ __forceinline__ void wit_level_gates(const WitArgs &a, const WitProver &o, const uint32_t *order, uint32_t lo, uint32_t inv_lo,
                                                uint32_t mid, uint32_t hi) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t t = lo + threadIdx.x; t < inv_lo; t += 256) wit_gate_lane_of<false, DIV>(a.w, order[t], o.aL, o.aR, o.aO, o.v, o.inputs, o.chi);
  if (INV && inv_lo < mid) {                                                                   // block-uniform
    const uint32_t first = inv_lo + threadIdx.x;
    const Fn run = wit_inv_forward(a.w, order, first, mid, 256, o.aL, o.aR, o.aO, o.v, o.chi);
    wit_inv_backward(order, first, mid, 256, inv(run), o.aL, o.aR, o.aO);
  }
  for (uint32_t t = mid + wave; t < hi; t += 4) {                                              // wave-uniform
    const uint32_t i = order[t];
    const uint32_t *rp = a.w.rows.row_ptr + 2 * (size_t)i;
    const Fn one = fe_one<FN>();
    const Fn left = wave_sum(fn_reduce(eval_row(a.w.rows, rp[0] + lane, rp[1], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
    const Fn right = wave_sum(fn_reduce(eval_row(a.w.rows, rp[1] + lane, rp[2], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
    if (DIV) {
      if (lane == 0) wit_gate_store_of<INV, DIV>(a.w.op[i], a.w.arg[i], left, right, o.inputs, o.aL + i, o.aR + i, o.aO + i);
    } else if (lane == 0) {
      const WitGate g = wit_gate_values_of<INV>(a.w.op[i], a.w.arg[i], left, right, o.inputs);
      wit_store(o.aL + i, g.L);
      wit_store(o.aR + i, g.R);
      wit_store(o.aO + i, g.O);
    }
  }
}
template <bool INV, bool DIV> __global__ void __launch_bounds__(256) k_witness_block(WitArgs a) {
  const WitProver o = wit_prover(a, blockIdx.x);
  for (uint32_t l = a.l_lo; l < a.l_hi; l++) {
    const uint32_t mid = a.w.level_long[l];
    wit_level_gates<INV, DIV>(a, o, a.w.order, a.w.level_ptr[l], INV ? a.w.level_inv[l] : mid, mid, a.w.level_ptr[l + 1]);
    if (l + 1 < a.l_hi) {
      __threadfence_block();
      __syncthreads();
    }
  }
}

// A block per prover over the COMPRESSED levels (kernels.h WitDev): at each level (A) its ordinary gates as k_witness_block runs
// them, heads of chains among them; a fence and a barrier; (B) the M members of all chains headed at this level as ONE segmented
// inclusive prefix product -- or, in a phase with an affine member, prefix composition of affine maps (witness_scan.cuh).  Thread t owns the run [t R, (t + 1) R) of R = ceil(M / 256) elements: a local pass,
// the scan of the 256 runs' parts -- within a wave by lane shuffles (Kogge-Stone, 6 steps), across the four waves through 4 parts in
// LDS -- and a second pass that applies the carry: 2 R + 10 dependent multiplications where the gates one by one take M levels.
// Barriers: M and the level range are the same for every thread of a launch, no thread returns early, and the shuffles run with all
// 64 lanes active (a thread whose run is empty carries the identity).  The LDS parts of one level are read before that level's
// closing barrier and written again only after it.
// k_witness_scan<AFFINE>: the same skeleton over either monoid -- WitPart under the product, or WitAff under the composition of
// affine maps for a phase that has an affine member (every level of such a phase runs the affine operator: a product member is the
// map with f = 0).  WitScanOf<AFFINE> is what the skeleton needs of a monoid; the parts in LDS are WORDS int32 each.
__device__ __forceinline__ Fn fn_shfl_up(const Fn &x, uint32_t off) {
  Fn r;
#pragma unroll
  for (int j = 0; j < NL; j++) r.v[j] = __shfl_up(x.v[j], off, 64);
  return r;
}
__device__ __forceinline__ Fn fn_select(bool take, const Fn &x, const Fn &y) {
  Fn r;
#pragma unroll
  for (int j = 0; j < NL; j++) r.v[j] = take ? x.v[j] : y.v[j];
  return r;
}
template <bool AFFINE> struct WitScanOf;
template <> struct WitScanOf<false> {
  using Part = WitPart;
  static constexpr int WORDS = NL + 1;
  static __device__ __forceinline__ Part identity() { return wit_part_identity(); }
  static __device__ __forceinline__ Part combine(const Part &a, const Part &b) { return wit_part_combine(a, b); }
  static __device__ __forceinline__ Part shfl_up(const Part &x, uint32_t off) { return {fn_shfl_up(x.v, off), __shfl_up(x.flag, off, 64)}; }
  static __device__ __forceinline__ Part select(bool take, const Part &x, const Part &y) {
    return {fn_select(take, x.v, y.v), take ? x.flag : y.flag};
  }
  static __device__ __forceinline__ void put(int32_t *d, const Part &x) { raw_put(d, x.v); d[NL] = (int32_t)x.flag; }
  static __device__ __forceinline__ Part get(const int32_t *s) { return {raw_get(s), (uint32_t)s[NL]}; }
  static __device__ __forceinline__ Part local(const WitDev &w, uint32_t lo, uint32_t hi, const WitPlanes &o) { return wit_scan_local(w, lo, hi, o); }
  static __device__ __forceinline__ void apply(const WitDev &w, uint32_t lo, uint32_t hi, const Part &carry, const WitPlanes &o) {
    wit_scan_apply(w, lo, hi, carry.v, o);
  }
};
template <> struct WitScanOf<true> {
  using Part = WitAff;
  static constexpr int WORDS = 2 * NL + 1;
  static __device__ __forceinline__ Part identity() { return wit_aff_identity(); }
  static __device__ __forceinline__ Part combine(const Part &a, const Part &b) { return wit_aff_combine(a, b); }
  static __device__ __forceinline__ Part shfl_up(const Part &x, uint32_t off) {
    return {fn_shfl_up(x.a, off), fn_shfl_up(x.b, off), __shfl_up(x.flag, off, 64)};
  }
  static __device__ __forceinline__ Part select(bool take, const Part &x, const Part &y) {
    return {fn_select(take, x.a, y.a), fn_select(take, x.b, y.b), take ? x.flag : y.flag};
  }
  static __device__ __forceinline__ void put(int32_t *d, const Part &x) { raw_put(d, x.a); raw_put(d + NL, x.b); d[2 * NL] = (int32_t)x.flag; }
  static __device__ __forceinline__ Part get(const int32_t *s) { return {raw_get(s), raw_get(s + NL), (uint32_t)s[2 * NL]}; }
  static __device__ __forceinline__ Part local(const WitDev &w, uint32_t lo, uint32_t hi, const WitPlanes &o) { return wit_aff_local(w, lo, hi, o); }
  static __device__ __forceinline__ void apply(const WitDev &w, uint32_t lo, uint32_t hi, const Part &carry, const WitPlanes &o) {
    wit_aff_apply(w, lo, hi, carry.b, o);
  }
};
template <bool AFFINE, bool INV, bool DIV> __global__ void __launch_bounds__(256) k_witness_scan(WitArgs a) {
  using S = WitScanOf<AFFINE>;
  using Part = typename S::Part;
  __shared__ int32_t s_part[4][S::WORDS];
  const WitProver o = wit_prover(a, blockIdx.x);
  const WitPlanes pl{o.aL, o.aR, o.aO, o.v, o.chi};
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t l = a.l_lo; l < a.l_hi; l++) {
    const uint32_t mid = a.w.scan_long[l];
    wit_level_gates<INV, DIV>(a, o, a.w.scan_order, a.w.scan_ptr[l], INV ? a.w.scan_inv[l] : mid, mid, a.w.scan_ptr[l + 1]);
    const uint32_t c_lo = a.w.chain_ptr[l], c_hi = a.w.chain_ptr[l + 1];                       // block-uniform
    if (c_lo < c_hi) {
      __threadfence_block();
      __syncthreads();
      const uint32_t run = (c_hi - c_lo + 255) / 256;
      const uint32_t e_lo = min(c_lo + threadIdx.x * run, c_hi), e_hi = min(e_lo + run, c_hi);  // (M < 2^25: no wrap)
      Part x = S::local(a.w, e_lo, e_hi, pl);
#pragma unroll 1
      for (uint32_t off = 1; off < 64; off <<= 1) {
        const Part both = S::combine(S::shfl_up(x, off), x);
        x = S::select(lane >= off, both, x);
      }
      if (lane == 63) S::put(s_part[wave], x);
      const Part before = S::select(lane != 0, S::shfl_up(x, 1), S::identity());               // this wave's lanes below
      __syncthreads();
      Part carry = S::identity();
      for (uint32_t k = 0; k < wave; k++) carry = S::combine(carry, S::get(s_part[k]));
      carry = S::combine(carry, before);
      S::apply(a.w, e_lo, e_hi, carry, pl);
    }
    if (l + 1 < a.l_hi) {
      __threadfence_block();
      __syncthreads();
    }
  }
}
template <bool INV, bool DIV> static void (*wit_kernel_of(int form))(WitArgs) {
  if (form == 4) return k_witness_scan<true, INV, DIV>;
  if (form == 3) return k_witness_scan<false, INV, DIV>;
  if (form == 2) return k_witness_block<INV, DIV>;
  return k_witness_lane<INV, DIV>;
}
void witness_eval(hipStream_t st, const WitDev &w, size_t nb, int form, bool inv, bool div, uint32_t g_lo, uint32_t g_hi, uint32_t l_lo,
                  uint32_t l_hi, Words8 *aL, Words8 *aR, Words8 *aO, const Words8 *v, const Words8 *inputs, const Words8 *chi) {
  if (!nb || g_lo >= g_hi) return;
  const WitArgs a{w, nb, g_lo, g_hi, l_lo, l_hi, aL, aR, aO, v, inputs, chi};
  const dim3 blocks((unsigned)nb), lanes((unsigned)((nb + 255) / 256));
  void (*kernel)(WitArgs) = div ? (inv ? wit_kernel_of<true, true>(form) : wit_kernel_of<false, true>(form))
                                 : (inv ? wit_kernel_of<true, false>(form) : wit_kernel_of<false, false>(form));
  hipLaunchKernelGGL(kernel, form >= 2 ? blocks : lanes, dim3(256), 0, st, a);
}

// ---- the callers' ark planes in and out: a lane per (prover, scalar) ---------------------------------------------------------------
__device__ __forceinline__ Fn wit_const(const int32_t (&c)[NL]) {
  Fn r;
#pragma unroll
  for (int j = 0; j < NL; j++) r.v[j] = c[j];
  return r;
}
__global__ void __launch_bounds__(256) k_witness_convert(bool to_ark, size_t nb, size_t count, const Words8 *src, size_t src_stride,
                                                         Words8 *dst, size_t dst_stride, int *bad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb * count) return;
  const size_t p = i / count, k = i % count;
  const Words8 *in = src + p * src_stride + k;
  Words8 *out = dst + p * dst_stride + k;
  constexpr int32_t CIN[NL] = FN_ARK_IN, COUT[NL] = FN_ARK_OUT;
  uint32_t w[8] = {};
  if (!words_canonical(in)) atomicOr(bad, 1);
  else pack(w, canon(mul(load_words(in), to_ark ? wit_const(COUT) : wit_const(CIN))));
#pragma unroll
  for (int j = 0; j < 8; j++) out->w[j] = w[j];
}
void witness_convert(hipStream_t st, bool to_ark, size_t nb, size_t count, const Words8 *src, size_t src_stride, Words8 *dst,
                     size_t dst_stride, int *bad) {
  const size_t tot = nb * count;
  if (tot) hipLaunchKernelGGL(k_witness_convert, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, to_ark, nb, count, src, src_stride,
                              dst, dst_stride, bad);
}

}  // namespace bpk
