// k_mpc_witness.hip -- the two-party prover's witness, one dependency level of a bpgpu_witness program per launch pair
// (MpcProver::multiply / allocate_multiplier, r1cs_mpc/mpc_prover.rs:183-282).  The gates of one level are independent, and each of
// their products needs an opening, so a level is one network round: the mask launch evaluates the level's rows on every plane and
// writes d = a_L - x, e = a_R - y; the host opens them; the combine launch stores a_O.  The gate and plane arithmetic is
// mpc_witness_dev.cuh's.  No barrier and no fence inside a launch: a level reads only lower levels (or the other phase), and those
// were stored by earlier launches on the same stream.  Measured (profiles/mpc_witness.log), one _mask + _combine pair of one party, device
// part with the operands' conversions: 1.957 ms for 256 proofs x 1 024 INPUT gates, 0.073 ms per level for 256 proofs of the
// 64-shuffle, 0.069 ms for one proof of a 300-gate level; levels with long rows and more than 256 proofs are UNMEASURED.
#include "mpc_witness_dev.cuh"

using namespace bp;

namespace bpk {

__device__ __forceinline__ MpcWitPlanes mpc_wit_planes(const MpcWitLevel &a, size_t v) {
  return {a.aL + v * a.w.n, a.aR + v * a.w.n, a.aO + v * a.w.n, a.v + v * a.w.m, a.inputs + v * a.w.ninp * 2, a.chi + (v / 3) * a.w.nchi};
}

// (virtual prover v = 3 p + k, position u of the level in order[]) flattened into x, u the fastest: the lanes of a wave walk adjacent
// gates of one plane.  The first short_blocks blocks take the gates without a long row, [lo, mid), a lane each; the others take the
// gates [mid, hi) a WAVE each (lane-strided terms, then wave_sum, as wit_level_gates).  A wave leaves whole or not at all: every
// shuffle runs with 64 lanes.
__global__ void __launch_bounds__(256) k_mpc_witness_mask(MpcWitLevel a, unsigned short_blocks) {
  const size_t nvirt = 3 * a.nb, G = a.hi - a.lo;
  if (blockIdx.x < short_blocks) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, gs = a.mid - a.lo;
    if (e >= nvirt * gs) return;
    const size_t v = e / gs;
    const uint32_t u = a.lo + (uint32_t)(e % gs), i = a.w.order[u];
    const int k = (int)(v % 3);
    const MpcWitPlanes o = mpc_wit_planes(a, v);
    mpc_wit_mask_gate(mpc_wit_rows(a.w, i, k, o), i, v / 3, k, G, a.w.slot[u], o, a.trip, a.masked);
  } else {
    const size_t e = ((size_t)blockIdx.x - short_blocks) * 4 + (threadIdx.x >> 6), gl = a.hi - a.mid;     // wave-uniform
    if (e >= nvirt * gl) return;
    const uint32_t lane = threadIdx.x & 63;
    const size_t v = e / gl;
    const uint32_t u = a.mid + (uint32_t)(e % gl), i = a.w.order[u];
    const int k = (int)(v % 3);
    const MpcWitPlanes o = mpc_wit_planes(a, v);
    const uint32_t *rp = a.w.rows.row_ptr + 2 * (size_t)i;
    const Fn one = mpc_wit_one(k);
    const Fn left = wave_sum(fn_reduce(eval_row(a.w.rows, rp[0] + lane, rp[1], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
    const Fn right = wave_sum(fn_reduce(eval_row(a.w.rows, rp[1] + lane, rp[2], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
    if (lane == 0) mpc_wit_mask_gate(mpc_wit_pair(a.w.op[i], a.w.arg[i], left, right, o.inputs), i, v / 3, k, G, a.w.slot[u], o, a.trip, a.masked);
  }
}
void mpc_witness_mask(hipStream_t st, const MpcWitLevel &a) {
  const size_t nvirt = 3 * a.nb, gs = a.mid - a.lo, gl = a.hi - a.mid;
  const size_t short_blocks = (nvirt * gs + 255) / 256, long_blocks = (nvirt * gl + 3) / 4;
  if (!(short_blocks + long_blocks)) return;
  hipLaunchKernelGGL(k_mpc_witness_mask, dim3((unsigned)(short_blocks + long_blocks)), dim3(256), 0, st, a, (unsigned)short_blocks);
}

// a lane per (virtual prover, slot t): a_O of the t-th gate of the level in ascending gate index
__global__ void __launch_bounds__(256) k_mpc_witness_combine(MpcWitLevel a, const Words8 *opened) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, G = a.hi - a.lo;
  if (e >= 3 * a.nb * G) return;
  const size_t v = e / G, t = e % G;
  mpc_wit_combine_gate(a.w.asc[a.lo + t], v / 3, (int)(v % 3), G, t, mpc_wit_planes(a, v), opened, a.trip);
}
void mpc_witness_combine(hipStream_t st, const MpcWitLevel &a, const Words8 *opened) {
  const size_t tot = 3 * a.nb * (a.hi - a.lo);
  if (tot) hipLaunchKernelGGL(k_mpc_witness_combine, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a, opened);
}

}  // namespace bpk
