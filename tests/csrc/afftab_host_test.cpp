// CPU build (g++ -fsanitize=undefined) of the affine table builder of ec29.cuh (afftab_build: {1..8} P of several points in
// three levels with one inversion per level), driven as the table lanes of k_verify_front drive it: entry 0 and the all-zero
// rows of identity points are laid down first, then the builder fills the rest.  Test infrastructure only.
#include <cstring>
#include "../../mpc_bulletproof_amd/csrc/ec29.cuh"
using namespace bp;

namespace {
constexpr int SE = 8;
template <int T> struct HostMem {
  mutable Aff rows[T][SE];
  mutable Fp prefix[4 * T];
  mutable int prefix_top = -1;
  Aff row(int j, int e) const { return rows[j][e]; }
  void put(int j, int e, const Aff &a) const { rows[j][e] = a; }
  Fp pre(int s) const { return prefix[s]; }
  void set_pre(int s, const Fp &x) const { prefix[s] = x; if (s > prefix_top) prefix_top = s; }
};
// pts: T x 64 boundary bytes (zeros = identity).  unchecked: take the coordinates as they are (no curve test), so that a test can
// hand the builder a point with a zero denominator.  skip: bits of identity points the builder is to pass over whole (the
// wave-uniform mask of the kernel); must be identity points.
// out: T x 8 x 64 boundary bytes; limbs: T x 8 x 18 raw limbs of the rows; returns 0 / 1 (a zero denominator was met), < 0 on bad input
template <int T> int run(const uint8_t *pts, int unchecked, unsigned skip, uint8_t *out, int32_t *limbs, int *prefix_slots) {
  HostMem<T> mem;
  unsigned dead = 0;
  for (int j = 0; j < T; j++) {
    uint32_t w[16];
    memcpy(w, pts + 64 * j, 64);
    Aff P;
    if (unchecked) {
      if (!words_lt_mod<FP>(w) || !words_lt_mod<FP>(w + 8)) return -1;
      P.x = to_mont(unpack<FP>(w));
      P.y = to_mont(unpack<FP>(w + 8));
      uint32_t o = 0;
      for (int t = 0; t < 16; t++) o |= w[t];
      if (o == 0) { P.x = fe_zero<FP>(); P.y = fe_zero<FP>(); }
    } else if (!aff_from_boundary(P, w)) return -1;
    const bool inf = aff_is_inf(P);
    if (inf) dead |= 1u << j;
    mem.put(j, 0, P);
    if (inf) for (int e = 1; e < SE; e++) mem.put(j, e, P);
  }
  if (skip & ~dead) return -2;
  const bool bad = afftab_build<T>(mem, skip, dead);
  for (int j = 0; j < T; j++)
    for (int e = 0; e < SE; e++) {
      uint32_t w[16];
      aff_to_boundary(w, mem.rows[j][e]);
      memcpy(out + 64 * (j * SE + e), w, 64);
      for (int t = 0; t < NL; t++) {
        limbs[(j * SE + e) * 2 * NL + t] = mem.rows[j][e].x.v[t];
        limbs[(j * SE + e) * 2 * NL + NL + t] = mem.rows[j][e].y.v[t];
      }
    }
  *prefix_slots = mem.prefix_top + 1;
  return bad ? 1 : 0;
}
}  // namespace

extern "C" int h29_afftab(int T, const uint8_t *pts, int unchecked, unsigned skip, uint8_t *out, int32_t *limbs, int *prefix_slots) {
  if (T == 4) return run<4>(pts, unchecked, skip, out, limbs, prefix_slots);
  if (T == 8) return run<8>(pts, unchecked, skip, out, limbs, prefix_slots);
  return -3;
}
