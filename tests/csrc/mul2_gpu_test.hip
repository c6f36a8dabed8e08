// GPU twin of mul2_host_test.cpp: mul2 of fe29.cuh through the DEVICE code path (the asm MAD chains, which the host build does not
// run) on raw limb vectors, and the point additions of ec29.cuh whose hot path takes its Y through it, one element per lane.
// Test infrastructure only -- never linked into the product.  Built by __graft_entry__.build() into tests/csrc/libmul2_gpu.so;
// tests/test_gpu_fused_products.py compares its outputs with Python big integers / the Python model.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../mpc_bulletproof_amd/csrc/ec29.cuh"
using namespace bp;

constexpr int M2_LANES = 256;

// out = canonical words of (value(a) value(b) + value(c) value(d)) / 2^261 mod p; abcd: 4 x 9 limbs per case.  One block of 256 lanes
// strides over the cases.  with_mul: out2 = canonical mul(a, b) beside it (the caller passes c = 0)
__global__ void __launch_bounds__(M2_LANES) k_mul2(const int32_t *abcd, uint32_t *out, uint32_t *out2, size_t n) {
  for (size_t i = threadIdx.x; i < n; i += M2_LANES) {
    Fp v[4];
    for (int t = 0; t < 4; t++)
      for (int j = 0; j < NL; j++) v[t].v[j] = abcd[(4 * i + t) * NL + j];
    uint32_t w[8];
    pack(w, canon(mul2(v[0], v[1], v[2], v[3])));
    for (int j = 0; j < 8; j++) out[8 * i + j] = w[j];
    if (out2) {
      pack(w, canon(mul(v[0], v[1])));
      for (int j = 0; j < 8; j++) out2[8 * i + j] = w[j];
    }
  }
}

__device__ Jac rescale(const Jac &p, uint32_t z0, uint32_t z1, uint32_t z2w) {   // (X z^2 : Y z^3 : Z z), the same point
  if (jac_is_inf(p)) return p;
  const uint32_t zw[8] = {z0, z1, z2w, 0, 0, 0, 0, 0};
  Fp z = to_mont(unpack<FP>(zw));
  Fp z2 = sqr(z), z3 = mul(z2, z);
  Jac r;
  r.X = mul(p.X, z2); r.Y = mul(p.Y, z3); r.Z = mul(p.Z, z);
  return r;
}
// the numbering of mul2_host_test.cpp (tests/fused_product_cases.py: POINT_OPS)
__global__ void __launch_bounds__(M2_LANES) k_point2(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int *rc, size_t n) {
  for (size_t i = threadIdx.x; i < n; i += M2_LANES) {
    uint32_t wa[16], wb[16];
    for (int j = 0; j < 16; j++) { wa[j] = a[16 * i + j]; wb[j] = b[16 * i + j]; }
    Aff p, q;
    if (!aff_from_boundary(p, wa) || !aff_from_boundary(q, wb)) { rc[i] = -1; continue; }
    Jac pj = jac_from_aff(p), r;
    if (op == 0) r = jac_madd(pj, q);
    else if (op == 1) r = jac_add(rescale(pj, 0x54321, 11, 5), rescale(jac_from_aff(q), 0x12345, 7, 9));
    else if (op == 3) r = xyzz_to_jac(xyzz_madd(xyzz_madd(xyzz_inf(), p), q));
    else if (op == 4 || op == 5) {
      if (aff_is_inf(q)) { rc[i] = -3; continue; }
      if (op == 4) r = xyzz_to_jac(xyzz_madd_nzq(xyzz_from_jac(rescale(pj, 0x54321, 11, 5)), q));
      else r = jac_madd_nzq(rescale(pj, 0x12345, 7, 9), q);
    } else { rc[i] = -2; continue; }
    uint32_t wo[16];
    aff_to_boundary(wo, jac_to_aff(r));
    for (int j = 0; j < 16; j++) out[16 * i + j] = wo[j];
    rc[i] = 0;
  }
}

namespace {
struct DevBuf {
  void *p = nullptr;
  explicit DevBuf(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) p = nullptr; }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
bool up(DevBuf &d, const void *h, size_t bytes) { return d.p && hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice) == hipSuccess; }
bool down(void *h, const DevBuf &d, size_t bytes) { return d.p && hipMemcpy(h, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
}  // namespace

extern "C" {
// both: 0 = ran, -100 = no HIP device / runtime error.  out2 may be null.
int m2g_mul2(const int32_t *abcd, size_t n, uint8_t *out, uint8_t *out2) {
  DevBuf din(4 * NL * 4 * n), dout(32 * n), dout2(32 * n);
  if (!up(din, abcd, 4 * NL * 4 * n) || !dout.p || !dout2.p) return -100;
  hipLaunchKernelGGL(k_mul2, dim3(1), dim3(M2_LANES), 0, 0, (const int32_t *)din.p, (uint32_t *)dout.p, out2 ? (uint32_t *)dout2.p : nullptr, n);
  if (hipDeviceSynchronize() != hipSuccess) return -100;
  if (out2 && !down(out2, dout2, 32 * n)) return -100;
  return down(out, dout, 32 * n) ? 0 : -100;
}
int m2g_point(int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out, int *rc) {
  DevBuf da(64 * n), db(64 * n), dout(64 * n), drc(4 * n);
  if (!up(da, a, 64 * n) || !up(db, b, 64 * n) || !dout.p || !drc.p) return -100;
  if (hipMemset(dout.p, 0, 64 * n) != hipSuccess) return -100;
  hipLaunchKernelGGL(k_point2, dim3(1), dim3(M2_LANES), 0, 0, op, (const uint32_t *)da.p, (const uint32_t *)db.p, (uint32_t *)dout.p, (int *)drc.p, n);
  if (hipDeviceSynchronize() != hipSuccess) return -100;
  return down(out, dout, 64 * n) && down(rc, drc, 4 * n) ? 0 : -100;
}
}
