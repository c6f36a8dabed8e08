// k_rows.hip -- constraint rows against witnesses: the row-major view of a resident circuit (built on the device from its column-
// major arrays) and the kernels of bpgpu_r1cs_constraints_satisfied / bpgpu_mpc_constraints_eval (Prover::constraints_satisfied,
// prover.rs:405-409; MpcProver::constraints_satisfied, mpc_prover.rs:538-568).  The arithmetic is eval_row of fn_dev.cuh.
#include "fn_dev.cuh"

using namespace bp;

namespace bpk {

// A row of up to ROWS_LANE_MAX terms is evaluated by one lane, a longer one by a wave (lane-strided terms, then wave_sum).  The route
// depends on the row's length alone.  DESIGN.md ("Constraint rows against witnesses") has the measurement behind the value.
#ifndef ROWS_LANE_MAX
#define ROWS_LANE_MAX 64
#endif
uint32_t rows_lane_max() { return ROWS_LANE_MAX; }

// ---- the view: count by constraint row, scan (csr_scan), scatter; then the list of long rows ----------------------------------------
// A lane per term.  A term's column is found by a binary search in col_ptr (the column-major arrays do not store it); its stored row
// j q + r belongs to constraint r with multiplier chi_j.
__global__ void __launch_bounds__(256) k_rows_count(const uint32_t *row, size_t nnz, size_t q, uint32_t *cnt) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nnz) return;
  atomicAdd(&cnt[row[t] % q + 1], 1u);
}
__global__ void __launch_bounds__(256) k_rows_scatter(CircuitDev c, const uint32_t *row_ptr, uint32_t *fill, uint32_t *var, Words8 *coeff) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= c.nnz) return;
  size_t lo = 0, hi = 3 * c.n + c.m + 1;            // the column o with col_ptr[o] <= t < col_ptr[o + 1]: lo <= o < hi
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (c.col_ptr[mid] <= t) lo = mid; else hi = mid;
  }
  const size_t o = lo;
  uint32_t kind, idx;
  if (o < 3 * c.n) { kind = (uint32_t)(o / c.n); idx = (uint32_t)(o % c.n); }
  else if (o < 3 * c.n + c.m) { kind = 3; idx = (uint32_t)(o - 3 * c.n); }
  else { kind = 4; idx = 0; }
  const uint32_t rr = c.row[t], r = (uint32_t)(rr % c.q), j = (uint32_t)(rr / c.q);
  const uint32_t pos = row_ptr[r] + atomicAdd(&fill[r], 1u);
  var[pos] = idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT;
  coeff[pos] = c.coeff[t];
}
__global__ void __launch_bounds__(256) k_rows_long(const uint32_t *row_ptr, size_t q, uint32_t *long_rows, uint32_t *nlong) {
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= q) return;
  if (row_ptr[r + 1] - row_ptr[r] > ROWS_LANE_MAX) long_rows[atomicAdd(nlong, 1u)] = (uint32_t)r;
}
// (nnz: a wave's lane-strided term index t + 64 must not wrap)
bool rows_view_supported(const CircuitDev &c) {
  return c.n <= ROWS_IDX_MASK && c.m <= ROWS_IDX_MASK && c.nchi < 16 && c.q < 0xFFFFFFFFu && c.nnz < 0xFFFFFF00u;
}
namespace {
// [coeff nnz | row_ptr q + 1 | var nnz | long_rows q | fill q | nlong], every part 256-byte aligned
struct ViewLayout { size_t coeff, row_ptr, var, long_rows, fill, nlong, total; };
size_t up256(size_t x) { return (x + 255) / 256 * 256; }
ViewLayout view_layout(const CircuitDev &c) {
  ViewLayout l;
  const size_t nnz = c.nnz ? c.nnz : 1, q = c.q ? c.q : 1;
  l.coeff = 0;
  l.row_ptr = up256(nnz * 32);
  l.var = l.row_ptr + up256((q + 1) * 4);
  l.long_rows = l.var + up256(nnz * 4);
  l.fill = l.long_rows + up256(q * 4);
  l.nlong = l.fill + up256(q * 4);
  l.total = l.nlong + 256;
  return l;
}
}  // namespace
size_t rows_view_bytes(const CircuitDev &c) { return view_layout(c).total; }
void rows_view_build(hipStream_t st, const CircuitDev &c, void *mem, RowsDev *view, const uint32_t **nlong_dev) {
  const ViewLayout l = view_layout(c);
  uint8_t *base = (uint8_t *)mem;
  Words8 *coeff = (Words8 *)(base + l.coeff);
  uint32_t *row_ptr = (uint32_t *)(base + l.row_ptr), *var = (uint32_t *)(base + l.var), *long_rows = (uint32_t *)(base + l.long_rows),
           *fill = (uint32_t *)(base + l.fill), *nlong = (uint32_t *)(base + l.nlong);
  (void)hipMemsetAsync(base + l.row_ptr, 0, l.var - l.row_ptr, st);
  (void)hipMemsetAsync(base + l.fill, 0, l.total - l.fill, st);        // fill and nlong
  if (c.q && c.nnz) {
    const unsigned tb = (unsigned)((c.nnz + 255) / 256);
    hipLaunchKernelGGL(k_rows_count, dim3(tb), dim3(256), 0, st, c.row, c.nnz, c.q, row_ptr);
    csr_scan(st, row_ptr, c.q + 1);
    hipLaunchKernelGGL(k_rows_scatter, dim3(tb), dim3(256), 0, st, c, (const uint32_t *)row_ptr, fill, var, coeff);
    hipLaunchKernelGGL(k_rows_long, dim3((unsigned)((c.q + 255) / 256)), dim3(256), 0, st, (const uint32_t *)row_ptr, c.q, long_rows, nlong);
  }
  view->row_ptr = row_ptr; view->var = var; view->coeff = coeff; view->long_rows = long_rows;
  view->q = c.q; view->nnz = c.nnz; view->nlong = 0;
  *nlong_dev = nlong;
}

// ---- evaluation: blocks [0, lane_blocks) hold a lane per (prover, row) and skip the long rows; the blocks after them a wave per
// (prover, long row) ----------------------------------------------------------------------------------------------------------------
struct RowsArgs {
  RowsDev v;
  size_t n, m, nchi, nvirt;
  int planes;
  const Words8 *aL, *aR, *aO, *vv, *chi;
  uint32_t *bad_row;
  Words8 *resid;
};
__device__ __forceinline__ Fn rows_part(const RowsArgs &a, size_t p, uint32_t lo, uint32_t hi, uint32_t step) {
  const Fn one = (a.planes == 1 || p % 3 == 2) ? fe_one<FN>() : fe_zero<FN>();
  return eval_row(a.v, lo, hi, step, a.aL + p * a.n, a.aR + p * a.n, a.aO + p * a.n, a.vv + p * a.m, one,
                  a.chi + p / (size_t)a.planes * a.nchi);
}
__device__ __forceinline__ void rows_finish(const RowsArgs &a, size_t p, uint32_t r, const Fn &e) {
  if (a.bad_row && !is_zero_exact(e)) atomicMin(&a.bad_row[p], r);
  if (a.resid) store_plain(&a.resid[p * a.v.q + r], e);
}
__global__ void __launch_bounds__(256) k_rows_eval(RowsArgs a, unsigned lane_blocks) {
  if (blockIdx.x < lane_blocks) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nvirt * a.v.q) return;
    const size_t p = i / a.v.q;
    const uint32_t r = (uint32_t)(i % a.v.q), lo = a.v.row_ptr[r], hi = a.v.row_ptr[r + 1];
    if (hi - lo > ROWS_LANE_MAX) return;
    rows_finish(a, p, r, fn_reduce(rows_part(a, p, lo, hi, 1)));
  } else {
    const size_t w = (size_t)(blockIdx.x - lane_blocks) * 4 + (threadIdx.x >> 6);       // wave-uniform from here on
    if (w >= a.nvirt * a.v.nlong) return;
    const size_t p = w / a.v.nlong;
    const uint32_t r = a.v.long_rows[w % a.v.nlong], lane = threadIdx.x & 63;
    const Fn e = wave_sum(fn_reduce(rows_part(a, p, a.v.row_ptr[r] + lane, a.v.row_ptr[r + 1], 64)));
    if (lane == 0) rows_finish(a, p, r, fn_reduce(e));
  }
}
namespace {
size_t rows_lane_blocks(const RowsDev &v, size_t nvirt) { return (nvirt * v.q + 255) / 256; }
size_t rows_wave_blocks(const RowsDev &v, size_t nvirt) { return (nvirt * v.nlong + 3) / 4; }
}  // namespace
bool rows_eval_fits(const RowsDev &v, size_t nvirt) {
  if (v.q && nvirt > ((size_t)1 << 38) / v.q) return false;
  return rows_lane_blocks(v, nvirt) + rows_wave_blocks(v, nvirt) < ((size_t)1 << 31);
}
void rows_eval(hipStream_t st, const RowsDev &v, size_t n, size_t m, size_t nchi, size_t nvirt, int planes, const Words8 *aL,
               const Words8 *aR, const Words8 *aO, const Words8 *vv, const Words8 *chi, uint32_t *bad_row, Words8 *resid) {
  if (!nvirt || !v.q) return;
  const RowsArgs a{v, n, m, nchi, nvirt, planes, aL, aR, aO, vv, chi, bad_row, resid};
  const unsigned lb = (unsigned)rows_lane_blocks(v, nvirt), wb = (unsigned)rows_wave_blocks(v, nvirt);
  hipLaunchKernelGGL(k_rows_eval, dim3(lb + wb), dim3(256), 0, st, a, lb);
}

// a lane per (prover, multiplier)
__global__ void __launch_bounds__(256) k_rows_gates(size_t tot, size_t n, const Words8 *aL, const Words8 *aR, const Words8 *aO, uint32_t *bad_gate) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= tot) return;
  const Fn e = sub(mul(load_plain(&aL[i]), load_plain(&aR[i])), load_plain(&aO[i]));
  if (!is_zero_exact(e)) atomicMin(&bad_gate[i / n], (uint32_t)(i % n));
}
void rows_gates(hipStream_t st, size_t nb, size_t n, const Words8 *aL, const Words8 *aR, const Words8 *aO, uint32_t *bad_gate) {
  const size_t tot = nb * n;
  if (tot) hipLaunchKernelGGL(k_rows_gates, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tot, n, aL, aR, aO, bad_gate);
}
__global__ void __launch_bounds__(256) k_rows_verdict(size_t nb, const uint32_t *bad_row, const uint32_t *bad_gate, int32_t *ok,
                                                      int64_t *first_row, int64_t *first_gate) {
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nb) return;
  const uint32_t br = bad_row[p], bg = bad_gate[p];
  ok[p] = (br == 0xFFFFFFFFu && bg == 0xFFFFFFFFu) ? 1 : 0;
  if (first_row) first_row[p] = br == 0xFFFFFFFFu ? -1 : (int64_t)br;
  if (first_gate) first_gate[p] = bg == 0xFFFFFFFFu ? -1 : (int64_t)bg;
}
void rows_verdict(hipStream_t st, size_t nb, const uint32_t *bad_row, const uint32_t *bad_gate, int32_t *ok, int64_t *first_row,
                  int64_t *first_gate) {
  if (nb) hipLaunchKernelGGL(k_rows_verdict, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, nb, bad_row, bad_gate, ok, first_row, first_gate);
}

}  // namespace bpk
