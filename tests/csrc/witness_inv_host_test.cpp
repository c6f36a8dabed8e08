// CPU build (g++ -fsanitize=undefined) of the INV gate of witness_dev.cuh, driven as the launch forms of k_witness.hip drive it: gate
// by gate in program order (wit_gate_lane: one inversion per gate), and level by level with T emulated threads, where thread t owns
// the short-row INV gates inv + t, inv + t + T, .. of a level and inverts ONCE for all of them (wit_inv_forward / wit_inv_backward),
// a long row is summed from 64 lane parts and inverted by wit_gate_values, and every other gate is wit_gate_lane_of<false>.  Reads
// gate programs from a file, prints one line per gate.  Test infrastructure only.
//
// Usage: witness_inv_host_test <case file> <T>.  Case file as tests/csrc/witness_host_test.cpp reads it, integers as hex: `ncases`,
// then per case `n m npairs nchi`, the nchi gadget challenges, the m values, the 2 npairs input values (all plain canonical), and per
// gate `op arg nleft nright` followed by nleft + nright terms `kind idx j coeff`.  Levels are taken over the whole program.
// Output per gate: a_L a_R a_O of the gate-by-gate form, then of the level form.
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
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "r");
  const uint32_t T = (uint32_t)atoi(argv[2]);
  if (!f || !T) return 2;
  unsigned ncases = 0;
  if (fscanf(f, "%x", &ncases) != 1) return 3;
  for (unsigned c = 0; c < ncases; c++) {
    unsigned n, m, npairs, nchi;
    if (fscanf(f, "%x %x %x %x", &n, &m, &npairs, &nchi) != 4) return 3;
    std::vector<Words8> chi(nchi + 1), vals(m + 1), pairs(2 * npairs + 1), coeff;
    std::vector<uint32_t> var, row_ptr(1, 0), arg(n + 1), level(n + 1, 0);
    std::vector<uint8_t> op(n + 1);
    for (unsigned i = 0; i < nchi; i++) if (!read_words(f, &chi[i])) return 4;
    for (unsigned i = 0; i < m; i++) if (!read_words(f, &vals[i])) return 4;
    for (unsigned i = 0; i < 2 * npairs; i++) if (!read_words(f, &pairs[i])) return 4;
    uint32_t levels = 0;
    for (unsigned i = 0; i < n; i++) {
      unsigned o, a, nl, nr;
      if (fscanf(f, "%x %x %x %x", &o, &a, &nl, &nr) != 4) return 3;
      if (o > WIT_OP_INV || o == 3 || (o == WIT_OP_BIT && a >= WIT_BIT_MAX) || (o == WIT_OP_INPUT && a >= npairs)) return 5;
      if ((o == WIT_OP_INV || o == WIT_OP_BIT) && nr) return 5;
      op[i] = (uint8_t)o;
      arg[i] = a;
      for (unsigned side = 0; side < 2; side++) {
        for (unsigned t = 0; t < (side ? nr : nl); t++) {
          unsigned kind, idx, j;
          Words8 cw, cm;
          if (fscanf(f, "%x %x %x", &kind, &idx, &j) != 3 || !read_words(f, &cw)) return 4;
          if (kind > 4 || (kind < 3 && idx >= i) || (kind == 3 && idx >= m) || j > nchi) return 5;
          if (kind < 3 && o != WIT_OP_INPUT) level[i] = std::max(level[i], level[idx] + 1);
          var.push_back(idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT);
          pack(cm.w, canon(to_mont(unpack<FN>(cw.w))));            // the handle keeps coefficients in Montgomery form
          coeff.push_back(cm);
        }
        row_ptr.push_back((uint32_t)var.size());
      }
      levels = std::max(levels, level[i] + 1);
    }
    if (row_ptr.size() != 2 * (size_t)n + 1) return 6;
    var.push_back(0);
    coeff.push_back(Words8{});
    WitDev w{};
    w.rows.row_ptr = row_ptr.data(); w.rows.var = var.data(); w.rows.coeff = coeff.data(); w.rows.q = 2 * n; w.rows.nnz = var.size() - 1;
    w.op = op.data(); w.arg = arg.data();
    w.n = n; w.m = m; w.nchi = nchi; w.ninp = npairs;
    std::vector<Words8> L(n + 1), R(n + 1), O(n + 1), L2(n + 1), R2(n + 1), O2(n + 1);
    // gate by gate, one inversion per INV gate
    for (unsigned i = 0; i < n; i++) wit_gate_lane(w, i, L.data(), R.data(), O.data(), vals.data(), pairs.data(), chi.data());
    // level by level: short rows, the INV gates among them last, then the long rows (the order bpgpu_witness_create stores)
    const Fn one = fe_one<FN>();
    for (uint32_t l = 0; l < levels; l++) {
      std::vector<uint32_t> order;
      uint32_t bound[4] = {0, 0, 0, 0};
      for (int list = 0; list < 3; list++) {
        bound[list] = (uint32_t)order.size();
        for (unsigned i = 0; i < n; i++) {
          if (level[i] != l) continue;
          const bool is_long = row_ptr[2 * i + 1] - row_ptr[2 * i] > LANE_MAX || row_ptr[2 * i + 2] - row_ptr[2 * i + 1] > LANE_MAX;
          if ((is_long ? 2 : (op[i] == WIT_OP_INV ? 1 : 0)) == list) order.push_back(i);
        }
      }
      bound[3] = (uint32_t)order.size();
      order.push_back(0);
      for (uint32_t t = bound[0]; t < bound[1]; t++)
        wit_gate_lane_of<false>(w, order[t], L2.data(), R2.data(), O2.data(), vals.data(), pairs.data(), chi.data());
      // every emulated thread runs its forward pass before any runs its backward pass, then the reverse order of threads: no thread
      // may depend on what another one stored
      std::vector<Fn> run(T);
      for (uint32_t t = 0; t < T; t++)
        run[t] = wit_inv_forward(w, order.data(), bound[1] + t, bound[2], T, L2.data(), R2.data(), O2.data(), vals.data(), chi.data());
      for (uint32_t t = T; t-- > 0;) wit_inv_backward(order.data(), bound[1] + t, bound[2], T, inv(run[t]), L2.data(), R2.data(), O2.data());
      for (uint32_t t = bound[2]; t < bound[3]; t++) {
        const uint32_t i = order[t];
        Fn left = fe_zero<FN>(), right = fe_zero<FN>();
        for (uint32_t lane = 0; lane < 64; lane++) {
          left = add(left, fn_reduce(eval_row(w.rows, row_ptr[2 * i] + lane, row_ptr[2 * i + 1], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
          right = add(right, fn_reduce(eval_row(w.rows, row_ptr[2 * i + 1] + lane, row_ptr[2 * i + 2], 64, L2.data(), R2.data(), O2.data(), vals.data(), one, chi.data())));
        }
        const WitGate g = wit_gate_values(op[i], arg[i], left, right, pairs.data());
        wit_store(&L2[i], g.L);
        wit_store(&R2[i], g.R);
        wit_store(&O2[i], g.O);
      }
    }
    for (unsigned i = 0; i < n; i++) {
      const Words8 *out[6] = {&L[i], &R[i], &O[i], &L2[i], &R2[i], &O2[i]};
      for (int k = 0; k < 6; k++) { print_words(*out[k]); printf(k == 5 ? "\n" : " "); }
    }
  }
  fclose(f);
  return 0;
}
