// pip2.cuh -- the plan and the per-lane bodies of k_pip2.hip's one-instance bucket pipeline, shared by k_pip2.hip (the
// stand-alone MSM and the combined batch check) and k_mixed.hip (the ragged combined check over proofs of several circuits).
#pragma once
#include "kernels.h"
#include "ec_dev.cuh"

namespace bpk {
using namespace bp;

constexpr uint32_t P2_TASK = 16;
constexpr uint32_t P2_NONE = 0xFFFFFFFFu;
constexpr uint32_t P2_HEAVY = 24;     // a bucket with more task partials than this is summed by a block of its own (K4b)

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct Pip2 {
  int c, W, half, bits;       // window bits, windows, buckets per window = 2^bits
  uint32_t K[9];              // sum_w 2^(c-1) 2^(c w)
  size_t n, nbk, max_tasks;
  const AffDev *pts;          // device Montgomery affine; zeros = identity
  const uint32_t *scalars;    // n x 8 plain canonical words
  const uint32_t *rho;        // optional: term i is multiplied by rho[i / rho_div] (plain canonical words)
  size_t rho_div;
  const uint32_t *rho_idx;    // optional, with rho: term i takes rho[rho_idx[i]] instead (proofs of different sizes in one instance)
  int *bad;
  uint32_t *keys, *sorted, *counts, *offsets, *cursor, *toffsets, *task_bucket;
  uint32_t *heavy;            // [0] = number of heavy buckets, [1..] their ids (written by K2)
  size_t max_heavy;
  JacRaw *partial, *buckets, *win;
};

static void p2_dims(size_t n, int c, size_t *W, size_t *nbk, size_t *mt) {
  *W = 252 / c + 1;
  *nbk = *W * ((size_t)1 << (c - 1));
  *mt = n * *W / P2_TASK + *nbk + 1;
}

static Pip2 p2_plan(const AffDev *pts, const uint32_t *scalars, size_t n, int c, void *scratch, int *bad) {
  Pip2 p{};
  size_t W, nbk, mt;
  p2_dims(n, c, &W, &nbk, &mt);
  p.c = c; p.W = (int)W; p.half = 1 << (c - 1); p.bits = c - 1;
  for (int j = 0; j < 9; j++) p.K[j] = 0;
  for (int w = 0; w < p.W; w++) { int bit = c * w + c - 1; p.K[bit >> 5] |= 1u << (bit & 31); }
  p.n = n; p.nbk = nbk; p.max_tasks = mt; p.pts = pts; p.scalars = scalars; p.bad = bad;
  uint8_t *q = (uint8_t *)scratch;
  p.keys = (uint32_t *)q; q += al(n * W * 4);
  p.sorted = (uint32_t *)q; q += al(n * W * 4);
  p.counts = (uint32_t *)q; q += al((nbk + 1) * 4);
  p.offsets = (uint32_t *)q; q += al((nbk + 1) * 4);
  p.cursor = (uint32_t *)q; q += al((nbk + 1) * 4);
  p.toffsets = (uint32_t *)q; q += al((nbk + 1) * 4);
  p.task_bucket = (uint32_t *)q; q += al(mt * 4);
  p.heavy = (uint32_t *)q; q += al((mt / P2_HEAVY + 2) * 4);
  p.max_heavy = mt / P2_HEAVY + 1;
  p.partial = (JacRaw *)q; q += al(mt * sizeof(JacRaw));
  p.buckets = (JacRaw *)q; q += al(nbk * sizeof(JacRaw));
  p.win = (JacRaw *)q;
  return p;
}

__device__ __forceinline__ int p2_digit(const uint32_t sp[9], int c, int w) {
  const int bit = c * w, k = bit >> 5, sft = bit & 31;
  uint64_t two = (uint64_t)sp[k] | (k + 1 < 9 ? (uint64_t)sp[k + 1] << 32 : 0);
  return (int)((two >> sft) & ((1u << c) - 1)) - (1 << (c - 1));
}

// atomicAdd(&base[b], 1) for the lanes with `valid`, returning each lane's old value -- with the lanes of a wave that hit the
// SAME counter combined into one atomic (up to 4 distinct counters per wave, the rest individually).  Low-entropy digits
// (the top window holds 252 mod c bits; equal scalars) otherwise serialise thousands of atomics on one address:
// 0.11 ms each in K1 and K3 of a 2^14-term MSM.
__device__ __forceinline__ uint32_t p2_agg_inc(uint32_t *base, uint32_t b, bool valid) {
  const int lane = (int)(threadIdx.x & 63);
  uint32_t res = 0;
  uint64_t todo = __ballot(valid);
#pragma unroll 1
  for (int it = 0; it < 4 && todo; it++) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t v = (uint32_t)__shfl((int)b, leader, 64);
    const uint64_t same = __ballot(valid && b == v) & todo;
    uint32_t old = 0;
    if (lane == leader) old = atomicAdd(&base[v], (uint32_t)__popcll(same));
    old = (uint32_t)__shfl((int)old, leader, 64);
    if ((same >> lane) & 1) res = old + (uint32_t)__popcll(same & ((1ull << lane) - 1));
    todo &= ~same;
  }
  if ((todo >> lane) & 1) res = atomicAdd(&base[b], 1u);
  return res;
}
// ---- K1: 256-thread blocks, lane per term
__device__ __forceinline__ void p2_digits_body(const Pip2 &p, size_t blk) {
  size_t i = blk * 256 + threadIdx.x;
  const bool live = i < p.n;            // whole waves stay in the loop below (wave-aggregated atomics)
  if (!live) i = p.n - 1;
  uint32_t any = 0;
#pragma unroll
  for (int t = 0; t < 16; t++) any |= p.pts[i].w[t];
  uint32_t s[8];
#pragma unroll
  for (int t = 0; t < 8; t++) s[t] = p.scalars[i * 8 + t];
  if (p.rho) {
    uint32_t r[8];
    const uint32_t *rp = p.rho + (size_t)(p.rho_idx ? p.rho_idx[i] : i / p.rho_div) * 8;
#pragma unroll
    for (int t = 0; t < 8; t++) r[t] = rp[t];
    if (live && (!words_lt_mod<FN>(r) || !words_lt_mod<FN>(s))) atomicOr(p.bad, 1);
    Fn x = mul(to_mont(unpack<FN>(s)), to_mont(unpack<FN>(r)));
    pack(s, from_mont(x));
  }
  uint32_t sp[9];
  uint64_t carry = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    uint64_t t = (uint64_t)(j < 8 ? s[j] : 0u) + p.K[j] + carry;
    sp[j] = (uint32_t)t;
    carry = t >> 32;
  }
  for (int w = 0; w < p.W; w++) {
    const int d = p2_digit(sp, p.c, w);
    uint32_t key = P2_NONE;
    const bool valid = live && d != 0 && any != 0;
    const uint32_t b = (uint32_t)w * (uint32_t)p.half + (uint32_t)((d < 0 ? -d : d) - 1);
    if (valid) key = b | (d < 0 ? 0x80000000u : 0u);
    (void)p2_agg_inc(p.counts, valid ? b : 0u, valid);
    if (live) p.keys[(size_t)w * p.n + i] = key;
  }
}
// ---- K4: 64-thread blocks, lane per task
__device__ __forceinline__ void p2_accum_body(const Pip2 &p, size_t blk) {
  const size_t t = blk * 64 + threadIdx.x;
  if (t >= p.toffsets[p.nbk]) return;
  const uint32_t b = p.task_bucket[t], slice = (uint32_t)t - p.toffsets[b];
  const uint32_t lo = p.offsets[b] + slice * P2_TASK, end = p.offsets[b + 1], hi = lo + P2_TASK < end ? lo + P2_TASK : end;
  Jac acc = jac_inf();
  // Two dependent loads per entry (index, then a random 64-byte row) against a ~1 650-instruction addition: the index
  // of entry e + 2 and the row of entry e + 1 are requested before the addition of entry e starts (with the row of
  // e + 1 waiting on an index fetched in the same iteration the launch ran at 60 percent of the addition rate).
  uint32_t cur[16], vcur = 0, vnxt = 0;
  if (lo < hi) {
    vcur = p.sorted[lo];
    const AffDev *src = &p.pts[vcur & 0x7FFFFFFFu];
#pragma unroll
    for (int j = 0; j < 16; j++) cur[j] = src->w[j];
    if (lo + 1 < hi) vnxt = p.sorted[lo + 1];
  }
  for (uint32_t e = lo; e < hi; e++) {
    uint32_t nxt[16], vnn = 0;
    if (e + 1 < hi) {
      const AffDev *src = &p.pts[vnxt & 0x7FFFFFFFu];
#pragma unroll
      for (int j = 0; j < 16; j++) nxt[j] = src->w[j];
      if (e + 2 < hi) vnn = p.sorted[e + 2];
    }
    Aff q;
    q.x = unpack<FP>(cur);
    q.y = unpack<FP>(cur + 8);
    if (vcur & 0x80000000u) q.y = neg(q.y);
    acc = jac_madd_nzq(acc, q);
#pragma unroll
    for (int j = 0; j < 16; j++) cur[j] = nxt[j];
    vcur = vnxt;
    vnxt = vnn;
  }
  raw_store(&p.partial[t], acc);
}

// K2..K6 of the combined check on a plan whose K1 has run (k_pip2.hip): scan, scatter, [bucket accumulation | ONE fixed-base
// MSM of 2 + 2 np generators with scalars fsum], heavy buckets, reduce, final (+ the fixed-base partial) -> out_xy boundary bytes.
// Profiling slots 13 (scan .. reduce) and 15 (final).
void p2_combined_tail(hipStream_t st, const Pip2 &p, const AffDev *table, size_t np, size_t cap, int c, const Words8 *fsum, JacRaw *fixed,
                      Words8 *out_xy, ProfMarkFn prof, void *prof_ctx);

}  // namespace bpk
