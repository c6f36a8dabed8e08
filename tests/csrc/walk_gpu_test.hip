// GPU harness of the generator walks of csrc/fixed_body.cuh on scalars the CALLER chooses: the verifier feeds fixed_chunk_body only
// scalars derived from its transcript, so the digits that start, empty and double a lane's accumulator cannot be placed through the
// C ABI.  Here a fixed-window table is built for any list of generators (identities among them) and the two bodies run over it:
// a proof per lane in runs of generators (fixed_chunk_body<C, 1>, what k_verify_back_q and k_fixed_msm_m launch) and 32 lanes per proof
// (fixed_small_body<C, 32>).  Test infrastructure only -- never linked into the product.  Built by __graft_entry__.build() into
// tests/csrc/libwalk_gpu.so; tests/test_gpu_walk_identity.py compares every output with the CPU oracle.
//
// The table is made WITHOUT the code under test: row e of window w of generator g is (e + 1) 2^(c w) G_g by Jacobian double-and-add
// (jac_dbl, jac_madd) and one inversion, nothing of the extended-Jacobian accumulators.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <new>
#include "../../mpc_bulletproof_amd/csrc/fixed_body.cuh"
using namespace bp;
using namespace bpk;

namespace {

// base[g * W + w] = 2^(c w) G_g (device affine; zeros for an identity generator); a lane per generator
template <int C>
__global__ void __launch_bounds__(64) k_bases(const uint32_t *gens /* ngens x 16 words, boundary */, AffDev *base, size_t ngens, int *bad) {
  constexpr int W = num_windows<C>();
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= ngens) return;
  uint32_t w16[16];
  for (int j = 0; j < 16; j++) w16[j] = gens[16 * g + j];
  Aff a;
  if (!aff_from_boundary(a, w16)) { *bad = 1; a.x = fe_zero<FP>(); a.y = fe_zero<FP>(); }
  Jac p = jac_from_aff(a);
  for (int w = 0; w < W; w++) {
    aff_store(&base[g * W + w], jac_to_aff(p));
    for (int i = 0; i < C; i++) p = jac_dbl(p);
  }
}
// table[(g * W + w) * HALF + e] = (e + 1) base[g * W + w]; a lane per row
template <int C>
__global__ void __launch_bounds__(64) k_rows(const AffDev *base, AffDev *table, size_t pages) {
  constexpr size_t HALF = (size_t)1 << (C - 1);
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= pages * HALF) return;
  const size_t page = i / HALF;
  const uint32_t k = (uint32_t)(i - page * HALF) + 1;       // 1 .. HALF
  const Aff b = aff_load(&base[page]);
  Jac acc = jac_inf();
  if (!aff_is_inf(b)) {
    for (int bit = C - 1; bit >= 0; bit--) {
      acc = jac_dbl(acc);
      if ((k >> bit) & 1) acc = jac_madd(acc, b);
    }
  }
  aff_store(&table[i], jac_to_aff(acc));
}
template <int C>
__global__ void __launch_bounds__(64) k_chunk_walk(const AffDev *table, size_t n, const uint32_t *scalars, JacRaw *part, size_t nb,
                                                   unsigned chunks, unsigned gens_per_chunk) {
  fixed_chunk_body<C, 1>(table, n, n, scalars, (2 + 2 * n) * 8, part, nb, chunks, gens_per_chunk, blockIdx.x);
}
template <int C>
__global__ void __launch_bounds__(64) k_small_walk(const AffDev *table, size_t n, const uint32_t *scalars, JacRaw *out, size_t nb) {
  fixed_small_body<C, 32>(table, n, n, scalars, (2 + 2 * n) * 8, out, nb, blockIdx.x);
}
__device__ void store_boundary(uint32_t *dst, Jac p) {
  if (!jac_is_inf(p) && is_zero_exact(p.Z)) p = jac_inf();
  uint32_t w[16];
  aff_to_boundary(w, jac_to_aff(p));
  for (int j = 0; j < 16; j++) dst[j] = w[j];
}
// every stored point as boundary bytes, and whether its Z limbs are literally zero (the stored form of the identity)
__global__ void __launch_bounds__(64) k_points_out(const JacRaw *in, uint32_t *out, int *zinf, size_t count) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const Jac p = raw_load(&in[i]);
  zinf[i] = jac_is_inf(p) ? 1 : 0;
  store_boundary(out + 16 * i, p);
}
// the partial sums of a proof added up as the verdict launch adds them (jac_add over raw partials)
__global__ void __launch_bounds__(64) k_parts_sum(const JacRaw *part, unsigned chunks, uint32_t *out, size_t nb) {
  const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= nb) return;
  Jac acc = raw_load(&part[p * chunks]);
  for (unsigned q = 1; q < chunks; q++) acc = jac_add(acc, raw_load(&part[p * chunks + q]));
  store_boundary(out + 16 * p, acc);
}

struct DevBuf {
  void *p = nullptr;
  explicit DevBuf(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) p = nullptr; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
};
bool up(DevBuf &d, const void *h, size_t bytes) { return d.p && hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice) == hipSuccess; }
bool down(void *h, const DevBuf &d, size_t bytes) { return d.p && hipMemcpy(h, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
unsigned blocks64(size_t n) { return (unsigned)((n + 63) / 64); }

struct WalkTable { int c; size_t ngens; DevBuf rows; WalkTable(int c_, size_t g, size_t bytes) : c(c_), ngens(g), rows(bytes) {} };

template <int C> int build_table(WalkTable &t, const uint8_t *gens) {
  constexpr int W = num_windows<C>();
  constexpr size_t HALF = (size_t)1 << (C - 1);
  const size_t pages = t.ngens * W;
  DevBuf dg(64 * t.ngens), base(sizeof(AffDev) * pages), bad(4);
  if (!up(dg, gens, 64 * t.ngens) || !base.p || !bad.p || hipMemset(bad.p, 0, 4) != hipSuccess) return -100;
  hipLaunchKernelGGL((k_bases<C>), dim3(blocks64(t.ngens)), dim3(64), 0, 0, (const uint32_t *)dg.p, (AffDev *)base.p, t.ngens, (int *)bad.p);
  hipLaunchKernelGGL((k_rows<C>), dim3(blocks64(pages * HALF)), dim3(64), 0, 0, (const AffDev *)base.p, (AffDev *)t.rows.p, pages);
  if (hipDeviceSynchronize() != hipSuccess) return -100;
  int b = 0;
  if (!down(&b, bad, 4)) return -100;
  return b ? -1 : 0;
}
// scalars below 2^252 keep every digit inside its page (the top window of either width then is a small positive digit)
bool scalars_in_range(const uint8_t *sc, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (sc[32 * i + 31] >= 0x10) return false;
  return true;
}
}  // namespace

extern "C" {
// generators: ngens x 64 boundary bytes (zeros = the identity).  c = 8 or 20.  nullptr: no device, no memory or a malformed point
void *wg_table_create(int c, const uint8_t *gens, size_t ngens) {
  if ((c != 8 && c != 20) || ngens < 4 || (ngens & 1)) return nullptr;
  const size_t pages = ngens * (size_t)(252 / c + 1), bytes = pages * ((size_t)1 << (c - 1)) * sizeof(AffDev);
  WalkTable *t = new (std::nothrow) WalkTable(c, ngens, bytes);
  if (!t) return nullptr;
  const int rc = !t->rows.p ? -100 : (c == 8 ? build_table<8>(*t, gens) : build_table<20>(*t, gens));
  if (rc != 0) { delete t; return nullptr; }
  return t;
}
void wg_table_destroy(void *h) { delete (WalkTable *)h; }
// fixed_chunk_body over nb proofs of 2 + 2n = ngens scalars (32 canonical bytes each), gens_per_chunk generators per wave.
// parts: nb x chunks x 64 bytes, part_inf: nb x chunks ints (stored Z all zero), sums: nb x 64 bytes.  0 = ran
int wg_chunk_walk(void *h, const uint8_t *scalars, size_t nb, unsigned gens_per_chunk, uint8_t *parts, int *part_inf, uint8_t *sums) {
  WalkTable *t = (WalkTable *)h;
  if (!t || !nb || !gens_per_chunk || !scalars_in_range(scalars, nb * t->ngens)) return -2;
  const size_t n = (t->ngens - 2) / 2;
  const unsigned chunks = (unsigned)((t->ngens + gens_per_chunk - 1) / gens_per_chunk);
  const size_t np = nb * chunks;
  DevBuf dsc(32 * nb * t->ngens), part(sizeof(JacRaw) * np), dout(64 * np), dinf(4 * np), dsum(64 * nb);
  if (!up(dsc, scalars, 32 * nb * t->ngens) || !part.p || !dout.p || !dinf.p || !dsum.p) return -100;
  if (hipMemset(part.p, 0xff, sizeof(JacRaw) * np) != hipSuccess) return -100;      // (a partial that is not written does not read as the identity)
  const dim3 grid(blocks64(nb) * chunks);
  if (t->c == 8) hipLaunchKernelGGL((k_chunk_walk<8>), grid, dim3(64), 0, 0, (const AffDev *)t->rows.p, n, (const uint32_t *)dsc.p, (JacRaw *)part.p, nb, chunks, gens_per_chunk);
  else hipLaunchKernelGGL((k_chunk_walk<20>), grid, dim3(64), 0, 0, (const AffDev *)t->rows.p, n, (const uint32_t *)dsc.p, (JacRaw *)part.p, nb, chunks, gens_per_chunk);
  hipLaunchKernelGGL(k_points_out, dim3(blocks64(np)), dim3(64), 0, 0, (const JacRaw *)part.p, (uint32_t *)dout.p, (int *)dinf.p, np);
  hipLaunchKernelGGL(k_parts_sum, dim3(blocks64(nb)), dim3(64), 0, 0, (const JacRaw *)part.p, chunks, (uint32_t *)dsum.p, nb);
  if (hipDeviceSynchronize() != hipSuccess) return -100;
  return down(parts, dout, 64 * np) && down(part_inf, dinf, 4 * np) && down(sums, dsum, 64 * nb) ? 0 : -100;
}
// fixed_small_body<C, 32>: out nb x 64 bytes
int wg_small_walk(void *h, const uint8_t *scalars, size_t nb, uint8_t *out) {
  WalkTable *t = (WalkTable *)h;
  if (!t || !nb || !scalars_in_range(scalars, nb * t->ngens)) return -2;
  const size_t n = (t->ngens - 2) / 2;
  DevBuf dsc(32 * nb * t->ngens), res(sizeof(JacRaw) * nb), dout(64 * nb), dinf(4 * nb);
  if (!up(dsc, scalars, 32 * nb * t->ngens) || !res.p || !dout.p || !dinf.p) return -100;
  if (hipMemset(res.p, 0xff, sizeof(JacRaw) * nb) != hipSuccess) return -100;
  const dim3 grid((unsigned)((nb + 1) / 2));
  if (t->c == 8) hipLaunchKernelGGL((k_small_walk<8>), grid, dim3(64), 0, 0, (const AffDev *)t->rows.p, n, (const uint32_t *)dsc.p, (JacRaw *)res.p, nb);
  else hipLaunchKernelGGL((k_small_walk<20>), grid, dim3(64), 0, 0, (const AffDev *)t->rows.p, n, (const uint32_t *)dsc.p, (JacRaw *)res.p, nb);
  hipLaunchKernelGGL(k_points_out, dim3(blocks64(nb)), dim3(64), 0, 0, (const JacRaw *)res.p, (uint32_t *)dout.p, (int *)dinf.p, nb);
  if (hipDeviceSynchronize() != hipSuccess) return -100;
  return down(out, dout, 64 * nb) ? 0 : -100;
}
}
