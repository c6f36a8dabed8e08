// CPU build (g++ -fsanitize=undefined) of the gate body of witness_dev.cuh (wit_gate_lane / wit_gate_values: what every lane of
// k_witness.hip runs), driven as the two launch forms drive it: a gate's rows by one lane, and each row spread over 64 lanes whose
// reduced parts are added before the gate's product.  Reads gate programs from a file, prints one line per gate.  Test
// infrastructure only.
//
// Case file, integers as hex: `ncases`, then per case `n m npairs nchi`, the nchi gadget challenges, the m values, the 2 npairs input
// values (all plain canonical), and per gate `op arg nleft nright` followed by nleft + nright terms `kind idx j coeff` (kind 0..2 read
// a_L / a_R / a_O of a gate below, kind 3 a value, kind 4 the constant; coeff plain canonical; an INPUT gate's arg is its pair).
// Output per gate: a_L a_R a_O of the lane form, then of the wave form.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/witness_dev.cuh"
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
    unsigned n, m, npairs, nchi;
    if (fscanf(f, "%x %x %x %x", &n, &m, &npairs, &nchi) != 4) return 3;
    std::vector<Words8> chi(nchi + 1), vals(m + 1), pairs(2 * npairs + 1), coeff(1);
    std::vector<uint32_t> var(1), row_ptr(1, 0), arg(n + 1);
    std::vector<uint8_t> op(n + 1);
    for (unsigned i = 0; i < nchi; i++) if (!read_words(f, &chi[i])) return 4;
    for (unsigned i = 0; i < m; i++) if (!read_words(f, &vals[i])) return 4;
    for (unsigned i = 0; i < 2 * npairs; i++) if (!read_words(f, &pairs[i])) return 4;
    coeff.clear();
    var.clear();
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
    if (row_ptr.size() != 2 * (size_t)n + 1) return 6;
    var.push_back(0);
    coeff.push_back(Words8{});
    WitDev w{};
    w.rows.row_ptr = row_ptr.data(); w.rows.var = var.data(); w.rows.coeff = coeff.data(); w.rows.q = 2 * n; w.rows.nnz = var.size() - 1;
    w.op = op.data(); w.arg = arg.data();
    w.n = n; w.m = m; w.nchi = nchi; w.ninp = npairs;
    std::vector<Words8> L(n + 1), R(n + 1), O(n + 1), L2(n + 1), R2(n + 1), O2(n + 1);
    const Fn one = fe_one<FN>();
    for (unsigned i = 0; i < n; i++) {
      // a lane per prover
      wit_gate_lane(w, i, L.data(), R.data(), O.data(), vals.data(), pairs.data(), chi.data());
      // a wave per gate: lane l takes the terms l, l + 64, .. of each row; the reduced parts are added, the gate reduces once more
      Fn left = fe_zero<FN>(), right = fe_zero<FN>();
      for (uint32_t l = 0; l < 64; l++) {
        left = add(left, fn_reduce(eval_row(w.rows, row_ptr[2 * i] + l, row_ptr[2 * i + 1], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
        right = add(right, fn_reduce(eval_row(w.rows, row_ptr[2 * i + 1] + l, row_ptr[2 * i + 2], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
      }
      const WitGate g = wit_gate_values(op[i], arg[i], left, right, pairs.data());
      wit_store(&L2[i], g.L);
      wit_store(&R2[i], g.R);
      wit_store(&O2[i], g.O);
      const Words8 *out[6] = {&L[i], &R[i], &O[i], &L2[i], &R2[i], &O2[i]};
      for (int k = 0; k < 6; k++) { print_words(*out[k]); printf(k == 5 ? "\n" : " "); }
    }
  }
  fclose(f);
  return 0;
}
