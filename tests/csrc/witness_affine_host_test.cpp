// CPU build (g++ -fsanitize=undefined) of the affine pieces of witness_scan.cuh (wit_aff_local, wit_aff_combine, wit_aff_apply: what
// every thread of k_witness_scan<true> runs), driven as that kernel drives them with T emulated threads in waves of W lanes: per
// extended compressed level the ordinary gates (wit_gate_lane), then the members as one segmented prefix composition of affine maps
// -- a local pass per thread, a Kogge-Stone scan of the parts inside each wave, the waves' totals combined in order, the carry
// applied.  Reads gate programs from a file, prints one line per gate.  Test infrastructure only.
//
// Case file, integers as hex: `ncases`, then per case `T W`, the case as tests/csrc/witness_host_test.cpp reads it (`n m npairs nchi`,
// challenges, values, input values, gates -- the rows as the library keeps them: an affine member's link term first in its link row),
// then `nlevels` and per level `ngates nelems`, the ordinary gates and the element words (gate | 1 << 25 on the first member of a
// chain | 1 << 26 where the link is the right row | 1 << 27 on an affine member).  Output per gate: a_L a_R a_O.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/witness_scan.cuh"
using namespace bp;
using namespace bpk;

namespace {
bool read_words(FILE *f, Words8 *out) {
  char s[80];
  if (fscanf(f, "%79s", s) != 1) return false;
  std::string h(s);
  if (h.size() > 64) return false;
  h = std::string(64 - h.size(), '0') + h;
  for (int j = 0; j < 8; j++) out->w[j] = (uint32_t)strtoul(h.substr(64 - 8 * (j + 1), 8).c_str(), nullptr, 16);
  return words_lt_mod<FN>(out->w);
}
void print_words(const Words8 &x) {
  for (int j = 7; j >= 0; j--) printf("%08x", x.w[j]);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned ncases = 0;
  if (fscanf(f, "%x", &ncases) != 1) return 3;
  for (unsigned c = 0; c < ncases; c++) {
    unsigned T, W, n, m, npairs, nchi;
    if (fscanf(f, "%x %x", &T, &W) != 2 || !T || !W || T % W) return 3;
    if (fscanf(f, "%x %x %x %x", &n, &m, &npairs, &nchi) != 4) return 3;
    std::vector<Words8> chi(nchi + 1), vals(m + 1), pairs(2 * npairs + 1), coeff;
    std::vector<uint32_t> var, row_ptr(1, 0), arg(n + 1);
    std::vector<uint8_t> op(n + 1);
    for (unsigned i = 0; i < nchi; i++) if (!read_words(f, &chi[i])) return 4;
    for (unsigned i = 0; i < m; i++) if (!read_words(f, &vals[i])) return 4;
    for (unsigned i = 0; i < 2 * npairs; i++) if (!read_words(f, &pairs[i])) return 4;
    for (unsigned i = 0; i < n; i++) {
      unsigned o, a, nl, nr;
      if (fscanf(f, "%x %x %x %x", &o, &a, &nl, &nr) != 4) return 3;
      if (o > WIT_OP_BIT || (o == WIT_OP_BIT && a >= WIT_BIT_MAX) || (o == WIT_OP_INPUT && a >= npairs)) return 5;
      op[i] = (uint8_t)o;
      arg[i] = a;
      for (unsigned side = 0; side < 2; side++) {
        for (unsigned t = 0; t < (side ? nr : nl); t++) {
          unsigned kind, idx, j;
          Words8 cw, cm;
          if (fscanf(f, "%x %x %x", &kind, &idx, &j) != 3 || !read_words(f, &cw)) return 4;
          if (kind > 4 || (kind < 3 && idx >= i) || (kind == 3 && idx >= m) || j > nchi) return 5;
          var.push_back(idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT);
          pack(cm.w, canon(to_mont(unpack<FN>(cw.w))));            // the handle keeps coefficients in Montgomery form
          coeff.push_back(cm);
        }
        row_ptr.push_back((uint32_t)var.size());
      }
    }
    var.push_back(0);
    coeff.push_back(Words8{});
    unsigned nlevels;
    if (fscanf(f, "%x", &nlevels) != 1) return 3;
    std::vector<uint32_t> gates, elems, gate_ptr(1, 0), elem_ptr(1, 0);
    for (unsigned l = 0; l < nlevels; l++) {
      unsigned ng, ne, x;
      if (fscanf(f, "%x %x", &ng, &ne) != 2) return 3;
      for (unsigned k = 0; k < ng; k++) { if (fscanf(f, "%x", &x) != 1 || x >= n) return 5; gates.push_back(x); }
      for (unsigned k = 0; k < ne; k++) {
        if (fscanf(f, "%x", &x) != 1 || (x & ROWS_IDX_MASK) >= n || x >> 28) return 5;
        const uint32_t i = x & ROWS_IDX_MASK, side = (x & WIT_ELEM_RIGHT) ? 1 : 0;
        const uint32_t lo = row_ptr[2 * i + side], len = row_ptr[2 * i + side + 1] - lo;
        // a link row starts with its link term; a product member's holds nothing else
        if (!len || ((var[lo] >> ROWS_KIND_SHIFT) & 7u) != 2 || (!(x & WIT_ELEM_AFFINE) && len != 1)) return 5;
        elems.push_back(x);
      }
      gate_ptr.push_back((uint32_t)gates.size());
      elem_ptr.push_back((uint32_t)elems.size());
    }
    if (gates.size() + elems.size() != n) return 6;
    elems.push_back(0);
    WitDev w{};
    w.rows.row_ptr = row_ptr.data(); w.rows.var = var.data(); w.rows.coeff = coeff.data(); w.rows.q = 2 * n; w.rows.nnz = var.size() - 1;
    w.op = op.data(); w.arg = arg.data(); w.chain_elem = elems.data();
    w.n = n; w.m = m; w.nchi = nchi; w.ninp = npairs;
    std::vector<Words8> L(n + 1), R(n + 1), O(n + 1);
    const WitPlanes pl{L.data(), R.data(), O.data(), vals.data(), chi.data()};
    std::vector<WitAff> part(T), scanned(T);
    for (unsigned l = 0; l < nlevels; l++) {
      for (uint32_t k = gate_ptr[l]; k < gate_ptr[l + 1]; k++)
        wit_gate_lane(w, gates[k], L.data(), R.data(), O.data(), vals.data(), pairs.data(), chi.data());
      const uint32_t c_lo = elem_ptr[l], c_hi = elem_ptr[l + 1];
      if (c_lo == c_hi) continue;
      const uint32_t run = (c_hi - c_lo + T - 1) / T;
      auto lo_of = [&](unsigned t) { const uint32_t x = c_lo + t * run; return x < c_hi ? x : c_hi; };
      auto hi_of = [&](unsigned t) { const uint32_t x = lo_of(t) + run; return x < c_hi ? x : c_hi; };
      for (unsigned t = 0; t < T; t++) part[t] = wit_aff_local(w, lo_of(t), hi_of(t), pl);
      for (unsigned off = 1; off < W; off <<= 1) {                 // every lane reads the step's inputs, then all write
        for (unsigned t = 0; t < T; t++) scanned[t] = t % W >= off ? wit_aff_combine(part[t - off], part[t]) : part[t];
        part = scanned;
      }
      for (unsigned t = 0; t < T; t++) {
        WitAff carry = wit_aff_identity();
        for (unsigned k = 0; k < t / W; k++) carry = wit_aff_combine(carry, part[k * W + W - 1]);
        carry = wit_aff_combine(carry, t % W ? part[t - 1] : wit_aff_identity());
        wit_aff_apply(w, lo_of(t), hi_of(t), carry.b, pl);
      }
    }
    for (unsigned i = 0; i < n; i++) {
      const Words8 *out[3] = {&L[i], &R[i], &O[i]};
      for (int k = 0; k < 3; k++) { print_words(*out[k]); printf(k == 2 ? "\n" : " "); }
    }
  }
  fclose(f);
  return 0;
}
