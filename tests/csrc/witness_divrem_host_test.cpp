// CPU build (g++ -fsanitize=undefined) of the integer division of csrc/int_div.cuh and of the DIVREM gate of witness_dev.cuh, driven as
// the launch forms of k_witness.hip drive it: gate by gate in program order (wit_gate_lane), and with every long row summed from 64
// lane parts and the gate stored by wit_gate_store_of, as a wave does it.  Test infrastructure only.
//
// Usage: witness_divrem_host_test prog <case file>: the case file as tests/csrc/witness_host_test.cpp reads it, integers as hex:
// `ncases`, then per case `n m npairs nchi`, the nchi gadget challenges, the m values, the 2 npairs input values (all plain canonical),
// and per gate `op arg nleft nright` followed by nleft + nright terms `kind idx j coeff`.  Output per gate: a_L a_R a_O of the
// gate-by-gate form, then of the wave form.
// witness_divrem_host_test div <pair file>: `npairs`, then per pair `x y`, any two integers below 2^256.  Output per pair: the
// quotient and the remainder of int_divrem.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/witness_dev.cuh"
using namespace bp;
using namespace bpk;

namespace {
constexpr uint32_t LANE_MAX = 64;        // rows_lane_max() of csrc/k_rows.hip
bool read_raw(FILE *f, Words8 *out) {
  char s[80];
  if (fscanf(f, "%79s", s) != 1) return false;
  std::string h(s);
  if (h.size() > 64) return false;
  h = std::string(64 - h.size(), '0') + h;
  for (int j = 0; j < 8; j++) out->w[j] = (uint32_t)strtoul(h.substr(64 - 8 * (j + 1), 8).c_str(), nullptr, 16);
  return true;
}
bool read_words(FILE *f, Words8 *out) { return read_raw(f, out) && words_lt_mod<FN>(out->w); }
void print_words(const uint32_t (&w)[8]) {
  for (int j = 7; j >= 0; j--) printf("%08x", w[j]);
}

int run_div(FILE *f) {
  unsigned npairs = 0;
  if (fscanf(f, "%x", &npairs) != 1) return 3;
  for (unsigned k = 0; k < npairs; k++) {
    Words8 x, y;
    if (!read_raw(f, &x) || !read_raw(f, &y)) return 4;
    uint32_t q[8], r[8];
    int_divrem(q, r, x.w, y.w);
    print_words(q);
    printf(" ");
    print_words(r);
    printf("\n");
  }
  return 0;
}

int run_prog(FILE *f) {
  unsigned ncases = 0;
  if (fscanf(f, "%x", &ncases) != 1) return 3;
  for (unsigned c = 0; c < ncases; c++) {
    unsigned n, m, npairs, nchi;
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
      if (o > WIT_OP_DIVREM || o == 3 || o == 5 || (o == WIT_OP_BIT && a >= WIT_BIT_MAX) || (o == WIT_OP_INPUT && a >= npairs)) return 5;
      if ((o == WIT_OP_INV || o == WIT_OP_BIT) && nr) return 5;
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
    for (unsigned i = 0; i < n; i++) wit_gate_lane(w, i, L.data(), R.data(), O.data(), vals.data(), pairs.data(), chi.data());
    // program order is topological: the short rows as a thread of the block form runs them, a long row as a wave and its lane 0
    const Fn one = fe_one<FN>();
    for (unsigned i = 0; i < n; i++) {
      const bool is_long = row_ptr[2 * i + 1] - row_ptr[2 * i] > LANE_MAX || row_ptr[2 * i + 2] - row_ptr[2 * i + 1] > LANE_MAX;
      if (!is_long) {
        wit_gate_lane_of<true, true>(w, i, L2.data(), R2.data(), O2.data(), vals.data(), pairs.data(), chi.data());
        continue;
      }
      Fn left = fe_zero<FN>(), right = fe_zero<FN>();
      for (uint32_t lane = 0; lane < 64; lane++) {
        left = add(left, fn_reduce(eval_row(w.rows, row_ptr[2 * i] + lane, row_ptr[2 * i + 1], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
        right = add(right, fn_reduce(eval_row(w.rows, row_ptr[2 * i + 1] + lane, row_ptr[2 * i + 2], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
      }
      wit_gate_store_of<true, true>(op[i], arg[i], left, right, pairs.data(), &L2[i], &R2[i], &O2[i]);
    }
    for (unsigned i = 0; i < n; i++) {
      const Words8 *out[6] = {&L[i], &R[i], &O[i], &L2[i], &R2[i], &O2[i]};
      for (int k = 0; k < 6; k++) { print_words(out[k]->w); printf(k == 5 ? "\n" : " "); }
    }
  }
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[2], "r");
  if (!f) return 2;
  int rc = 2;
  if (!strcmp(argv[1], "div")) rc = run_div(f);
  else if (!strcmp(argv[1], "prog")) rc = run_prog(f);
  fclose(f);
  return rc;
}
