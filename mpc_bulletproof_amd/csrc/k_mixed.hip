// k_mixed.hip -- the combined batch check over proofs of SEVERAL circuits: sum_p rho_p * mega_check_p as ONE point.
//
// Every proof's mega_check (r1cs/verifier.rs:516-547) uses the same B, B_blinding and a prefix G_0.., H_0.. of the resident
// generators, whatever its circuit: the generator scalars of all proofs add up into ONE fixed-base MSM over the common layout
// [B, B_blinding, G_0..G_{N-1}, H_0..H_{N-1}] (N = the largest padded n), and all proof points go into ONE bucket-method MSM.
// The chain keeps the shape of k_pip2.hip's verify_combined2; only the scalar assembly depends on a circuit:
//   1 front    [proof points of every segment: validate + convert, proof index per point | weights: gather, canonical?, zero? and the
//              gadget challenges canonical? | inversion pass of every segment's scalar assembly | zero the histogram]
//   2 scalars  k_verify_scalars (k_scalar.hip) per segment, into the segment's rows of the concatenated scalar buffers
//   3 K1       [digits of rho_p * s_{p,j} (p2_digits_body, weight by proof index) | generator column sums into the common layout]
//   4..8       k_pip2.hip's tail: scan, scatter, [bucket accumulation | the fixed-base MSM], heavy buckets, reduce, final
// A check that does not fit the one-instance pipeline (fewer than 256 or more than 2^16 proof points, or a generator count its
// fixed-base lanes do not take) keeps launches 1-3 and then runs the generic MSMs of bpgpu_r1cs_verify_combined.
// The segment table travels in the launches' kernel arguments (MIX_SEG_MAX entries): no copy command and no host wait per check.
#include "vs_prep.cuh"
#include "pip2.cuh"

using namespace bp;

namespace bpk {

struct MixFrontSeg {
  const Words8 *points, *rho, *chi;
  uint32_t pt_off, npts, p_off, nb, nvar, nchi, prep_blk, prep_nblk;
  VsPrepArgs prep;
};
struct MixFront {
  MixFrontSeg seg[MIX_SEG_MAX];
  uint32_t nseg, pb, rb, vb;          // blocks: proof points, weights, inversion passes (then the histogram reset)
  size_t tot, nbt;                     // proof points, proofs
  AffDev *pts; uint32_t *pidx; Words8 *rho_all;
  int *bad, *zero_rho;
  uint32_t *counts; size_t ncounts;
};
// the table travels by value: keep every launch's arguments inside HIP's 4 KB kernel-argument limit (MIX_SEG_MAX, VsPrepArgs, VerifyDims)
static_assert(sizeof(MixFront) <= 4096, "k_mix_front's arguments exceed 4 KB: lower MIX_SEG_MAX or pass the table in device memory");
__global__ void __launch_bounds__(256) k_mix_front(MixFront a) {
  const unsigned b = blockIdx.x;
  if (b < a.pb) {                                   // proof points (segment-major, proof-major inside a segment)
    const size_t i = (size_t)b * 256 + threadIdx.x;
    if (i >= a.tot) return;
    uint32_t s = 0;
    while (s + 1 < a.nseg && i >= a.seg[s + 1].pt_off) s++;
    const MixFrontSeg &g = a.seg[s];
    const size_t j = i - g.pt_off;
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 8; t++) { w[t] = g.points[2 * j].w[t]; w[8 + t] = g.points[2 * j + 1].w[t]; }
    Aff q;
    if (!aff_from_boundary(q, w)) { atomicOr(a.bad, 1); q.x = fe_zero<FP>(); q.y = fe_zero<FP>(); }
    aff_store(&a.pts[i], q);
    a.pidx[i] = g.p_off + (uint32_t)(j / g.nvar);
  } else if (b < a.pb + a.rb) {                     // weights and gadget challenges, lane per proof
    const size_t p = (size_t)(b - a.pb) * 256 + threadIdx.x;
    if (p >= a.nbt) return;
    uint32_t s = 0;
    while (s + 1 < a.nseg && p >= a.seg[s + 1].p_off) s++;
    const MixFrontSeg &g = a.seg[s];
    const size_t j = p - g.p_off;
    uint32_t r[8], any = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) { r[t] = g.rho[j].w[t]; any |= r[t]; a.rho_all[p].w[t] = r[t]; }
    if (!words_lt_mod<FN>(r)) atomicOr(a.bad, 1);
    if (!any && a.zero_rho) atomicOr(a.zero_rho, 1);
    for (uint32_t c = 0; c < g.nchi; c++)
      if (!words_canonical(&g.chi[j * g.nchi + c])) atomicOr(a.bad, 1);
  } else if (b < a.pb + a.rb + a.vb) {              // inversion pass of the segments whose assembly takes it here, lane per proof
    const uint32_t v = b - a.pb - a.rb;
    uint32_t s = 0;
    while (s < a.nseg && !(v >= a.seg[s].prep_blk && v < a.seg[s].prep_blk + a.seg[s].prep_nblk)) s++;
    if (s == a.nseg) return;
    vs_prep_lane(a.seg[s].prep, (size_t)(v - a.seg[s].prep_blk) * 256 + threadIdx.x);
  } else {                                          // histogram reset
    const size_t i = (size_t)(b - a.pb - a.rb - a.vb) * 256 + threadIdx.x;
    if (i < a.ncounts) a.counts[i] = 0;
  }
}

// generator column sums into the common layout: column j of [B, B_blinding, G_0..G_{N-1}, H_0..H_{N-1}] takes, from a segment of
// padded n = np (its rows laid out [B, B_blinding, G_0..G_{np-1}, H_0..H_{np-1}]), row entry j (j < 2 + N, G_{j-2} with j - 2 < np)
// or 2 + np + (j - 2 - N) (H); columns beyond a segment's np take nothing from it
struct MixColSeg { const Words8 *fixed; uint32_t p_off, nb, np; };
struct MixColsum { MixColSeg seg[MIX_SEG_MAX]; uint32_t nseg; size_t nmax; const Words8 *rho_all; Words8 *out; };
__device__ __forceinline__ void mix_colsum_body(const MixColsum &a, size_t j) {
  Fn acc = fe_zero<FN>();
  int cnt = 0;
  for (uint32_t s = 0; s < a.nseg; s++) {
    const MixColSeg &g = a.seg[s];
    size_t col;
    if (j < 2) col = j;
    else if (j < 2 + a.nmax) { if (j - 2 >= g.np) continue; col = j; }
    else { if (j - 2 - a.nmax >= g.np) continue; col = j - a.nmax + g.np; }
    const size_t nfix = 2 + 2 * (size_t)g.np;
    for (size_t p = threadIdx.x; p < g.nb; p += 256) {
      acc = add(acc, mul(load_plain(&g.fixed[p * nfix + col]), load_plain(&a.rho_all[g.p_off + p])));
      if ((++cnt & 15) == 0) acc = fn_reduce(acc);
    }
  }
  const Fn t = block_sum<256>(acc);
  if (threadIdx.x == 0) store_plain(&a.out[j], t);
}
static_assert(sizeof(Pip2) + sizeof(unsigned) + sizeof(MixColsum) + 16 <= 4096, "k_mix_k1's arguments exceed 4 KB");
__global__ void __launch_bounds__(256) k_mix_k1(Pip2 p, unsigned digit_blocks, MixColsum cs) {
  if (blockIdx.x < digit_blocks) p2_digits_body(p, blockIdx.x);
  else mix_colsum_body(cs, blockIdx.x - digit_blocks);
}
// generic route: var[i] *= rho_all[pidx[i]]
__global__ void __launch_bounds__(256) k_mix_scale(Words8 *var, const uint32_t *pidx, const Words8 *rho_all, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  store_plain(&var[i], mul(load_plain(&var[i]), load_plain(&rho_all[pidx[i]])));
}
__global__ void k_mix_poison(const int *bad, Words8 *out) {
  if (*bad && threadIdx.x < 16) out[threadIdx.x / 8].w[threadIdx.x % 8] = 0xFFFFFFFFu;
}

// ---- host side
namespace {
struct MixLayout {
  size_t tot = 0, nbt = 0, nmax = 1, nfix_all = 0, zpow_ints = 0;
  bool pip2 = false;
  int cw = 0;
};
MixLayout mix_layout(const MixSegIn *seg, size_t nseg, int c) {
  MixLayout l;
  for (size_t s = 0; s < nseg; s++) {
    l.tot += seg[s].d.nb * seg[s].nvar;
    l.nbt += seg[s].d.nb;
    if (seg[s].d.padded_n > l.nmax) l.nmax = seg[s].d.padded_n;
    l.nfix_all += seg[s].d.nb * (2 + 2 * seg[s].d.padded_n);
    l.zpow_ints += (verify_scalars_scratch_ints(seg[s].circ, seg[s].d) + 63) / 64 * 64;
  }
  l.pip2 = verify_combined2_supported(l.tot, 1, c, l.nmax);
  l.cw = l.pip2 ? pippenger2_window(l.tot) : pippenger_window(l.tot);
  return l;
}
// generic route: the fixed-base MSM's partial sums (fixed_msm_chunks of one MSM over 2 + 2N generators)
size_t mix_route_bytes(const MixLayout &l, int c) {
  if (l.pip2) return pippenger2_scratch_bytes(l.tot, l.cw);
  return al(fixed_msm_chunks(c, l.nmax, 1) * sizeof(JacRaw)) + pippenger_scratch_bytes(l.tot, l.cw);
}
}  // namespace

size_t verify_mixed_scratch_bytes(const MixSegIn *seg, size_t nseg, int c) {
  const MixLayout l = mix_layout(seg, nseg, c);
  return al(l.tot * sizeof(AffDev)) + al(l.tot * 4) + al(l.nbt * 32) + al(l.tot * 32) + al(l.nfix_all * 32) + al((2 + 2 * l.nmax) * 32) +
         al(3 * sizeof(JacRaw)) + al(l.zpow_ints * 4) + mix_route_bytes(l, c);
}

void verify_mixed(hipStream_t st, const MixedArgs &a) {
  const MixLayout l = mix_layout(a.seg, a.nseg, a.c);
  if (!l.nbt) return;
  uint8_t *q = (uint8_t *)a.scratch;
  AffDev *dpts = (AffDev *)q; q += al(l.tot * sizeof(AffDev));
  uint32_t *pidx = (uint32_t *)q; q += al(l.tot * 4);
  Words8 *rho_all = (Words8 *)q; q += al(l.nbt * 32);
  Words8 *var_sc = (Words8 *)q; q += al(l.tot * 32);
  Words8 *fixed_sc = (Words8 *)q; q += al(l.nfix_all * 32);
  const size_t nfix = 2 + 2 * l.nmax;
  Words8 *fsum = (Words8 *)q; q += al(nfix * 32);
  JacRaw *dtwo = (JacRaw *)q; q += al(3 * sizeof(JacRaw));
  int32_t *zpow = (int32_t *)q; q += al(l.zpow_ints * 4);
  Pip2 p{};
  if (l.pip2) {
    p = p2_plan(dpts, (const uint32_t *)var_sc, l.tot, l.cw, q, a.bad);
    p.rho = (const uint32_t *)rho_all; p.rho_div = 1; p.rho_idx = pidx;
  }
  // per-segment offsets, the scalar assembly's arguments and the front's table
  MixFront fr{};
  MixColsum cs{};
  struct SegRun { VerifyDims d; Words8 *fixed, *var; int32_t *zpow; bool fuse, fast; } run[MIX_SEG_MAX];
  size_t pt_off = 0, p_off = 0, fix_off = 0, z_off = 0;
  unsigned vb = 0;
  for (size_t s = 0; s < a.nseg; s++) {
    const MixSegIn &g = a.seg[s];
    SegRun &r = run[s];
    r.d = g.d;
    r.fixed = fixed_sc + fix_off;
    r.var = var_sc + pt_off;
    r.zpow = zpow + z_off;
    int32_t *aux = nullptr;
    size_t aux_stride = 0;
    r.fuse = verify_scalars_aux(g.circ, r.d, r.zpow, &aux, &aux_stride);
    r.fast = r.fuse && verify_scalars_fast_shape(g.circ, r.d);
    MixFrontSeg &f = fr.seg[s];
    f.points = g.points; f.rho = g.rho; f.chi = g.d.chi;
    f.pt_off = (uint32_t)pt_off; f.npts = (uint32_t)(g.d.nb * g.nvar); f.p_off = (uint32_t)p_off; f.nb = (uint32_t)g.d.nb;
    f.nvar = (uint32_t)g.nvar; f.nchi = (uint32_t)g.nchi;
    f.prep_blk = vb; f.prep_nblk = r.fuse ? (uint32_t)((g.d.nb + 255) / 256) : 0u;
    vb += f.prep_nblk;
    f.prep = VsPrepArgs{r.d, g.challenges, aux, aux_stride};
    if (r.fast) { f.prep.proof_scalars = g.proof_scalars; f.prep.fixed_sc = r.fixed; f.prep.var_sc = r.var; }
    cs.seg[s] = MixColSeg{r.fixed, (uint32_t)p_off, (uint32_t)g.d.nb, (uint32_t)g.d.padded_n};
    pt_off += g.d.nb * g.nvar;
    p_off += g.d.nb;
    fix_off += g.d.nb * (2 + 2 * g.d.padded_n);
    z_off += (verify_scalars_scratch_ints(g.circ, g.d) + 63) / 64 * 64;
  }
  fr.nseg = (uint32_t)a.nseg;
  fr.pb = (unsigned)((l.tot + 255) / 256);
  fr.rb = (unsigned)((l.nbt + 255) / 256);
  fr.vb = vb;
  fr.tot = l.tot; fr.nbt = l.nbt;
  fr.pts = dpts; fr.pidx = pidx; fr.rho_all = rho_all; fr.bad = a.bad; fr.zero_rho = a.zero_rho;
  fr.counts = l.pip2 ? p.counts : nullptr; fr.ncounts = l.pip2 ? p.nbk + 1 : 0;
  cs.nseg = (uint32_t)a.nseg; cs.nmax = l.nmax; cs.rho_all = rho_all; cs.out = fsum;
  { ProfMark pm(a.prof, a.prof_ctx, 12, st);
    // 1 front
    hipLaunchKernelGGL(k_mix_front, dim3(fr.pb + fr.rb + fr.vb + (unsigned)((fr.ncounts + 255) / 256)), dim3(256), 0, st, fr);
    // 2 scalars, one launch per segment (canonicity of the challenges / proof scalars is checked inside; weights and gadget
    // challenges in the front)
    for (size_t s = 0; s < a.nseg; s++) {
      const MixSegIn &g = a.seg[s];
      verify_scalars(st, g.circ, run[s].d, g.challenges, g.proof_scalars, run[s].fixed, run[s].var, nullptr, run[s].zpow, a.bad, nullptr,
                     run[s].fuse, run[s].fast);
    }
    // 3 K1: digits (pip2 route) | column sums
    const unsigned db = l.pip2 ? (unsigned)((l.tot + 255) / 256) : 0u;
    hipLaunchKernelGGL(k_mix_k1, dim3(db + (unsigned)nfix), dim3(256), 0, st, p, db, cs); }
  if (l.pip2) {
    p2_combined_tail(st, p, a.table, l.nmax, a.cap, a.c, fsum, dtwo, a.partial_xy, a.prof, a.prof_ctx);
    return;
  }
  // generic route (bpgpu_r1cs_verify_combined's sequence, on one stream): the ONE fixed-base MSM, the weighted proof-point MSM
  { ProfMark pm(a.prof, a.prof_ctx, 13, st);
    const size_t chunks = fixed_msm_chunks(a.c, l.nmax, 1);
    JacRaw *parts = (JacRaw *)q;
    fixed_msm(st, a.c, a.table, l.nmax, a.cap, (const uint32_t *)fsum, nfix * 8, dtwo, 1, chunks > 1 ? parts : nullptr);
    q += al(chunks * sizeof(JacRaw));
    hipLaunchKernelGGL(k_mix_scale, dim3((unsigned)((l.tot + 255) / 256)), dim3(256), 0, st, var_sc, (const uint32_t *)pidx,
                       (const Words8 *)rho_all, l.tot);
    pippenger(st, dpts, (const uint32_t *)var_sc, l.tot, l.cw, dtwo + 1, q); }
  { ProfMark pm(a.prof, a.prof_ctx, 15, st);
    segmented_sum(st, dtwo, dtwo + 2, 1, 2);
    jac_to_boundary(st, dtwo + 2, a.partial_xy, 1); }
}

void mixed_poison(hipStream_t st, const int *bad, Words8 *out_xy) {
  hipLaunchKernelGGL(k_mix_poison, dim3(1), dim3(64), 0, st, bad, out_xy);
}

}  // namespace bpk
