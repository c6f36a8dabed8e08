// CPU build (g++ -fsanitize=undefined) of the gate and plane arithmetic of mpc_witness_dev.cuh (what every lane of k_mpc_witness.hip
// runs), driven level by level as the two launches drive it, for ONE party's three planes of one proof: the mask step with a gate's
// rows by one lane, and with each row spread over 64 lanes whose reduced parts are added (the wave form), then the combine step.
// Reads programs, planes, triples and opened values from a file, prints one line per (level, plane, slot).  Test infrastructure only.
//
// Case file, integers as hex, values plain canonical: `ncases`, then per case `n m npairs nchi nlevels`, the nchi gadget challenges,
// per plane k = 0, 1, 2 the m values and the 2 npairs input values, per gate `op arg nleft nright` followed by nleft + nright terms
// `kind idx j coeff` (as tests/csrc/witness_host_test.cpp), and per level `G`, the G gates in ascending index, the triples
// [x, y, z][k][slot] and the opened [d, e][slot].
// Output per (level, plane, slot): a_L a_R d e a_O of the lane form, then of the wave form.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/mpc_witness_dev.cuh"
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
    unsigned n, m, npairs, nchi, nlevels;
    if (fscanf(f, "%x %x %x %x %x", &n, &m, &npairs, &nchi, &nlevels) != 5) return 3;
    std::vector<Words8> chi(nchi + 1), vals(3 * m + 1), pairs(6 * npairs + 1), coeff;
    std::vector<uint32_t> var, row_ptr(1, 0), arg(n + 1);
    std::vector<uint8_t> op(n + 1);
    for (unsigned i = 0; i < nchi; i++) if (!read_words(f, &chi[i])) return 4;
    for (unsigned k = 0; k < 3; k++) {
      for (unsigned i = 0; i < m; i++) if (!read_words(f, &vals[k * m + i])) return 4;
      for (unsigned i = 0; i < 2 * npairs; i++) if (!read_words(f, &pairs[k * 2 * npairs + i])) return 4;
    }
    for (unsigned i = 0; i < n; i++) {
      unsigned o, a, nl, nr;
      if (fscanf(f, "%x %x %x %x", &o, &a, &nl, &nr) != 4) return 3;
      if (o > WIT_OP_INPUT || (o == WIT_OP_INPUT && a >= npairs)) return 5;      // (a BIT gate has no place on shares)
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
    // the planes of the three virtual provers, for the lane form and for the wave form
    std::vector<Words8> P[2][3];
    for (int form = 0; form < 2; form++) for (int a = 0; a < 3; a++) P[form][a].assign(3 * (size_t)n + 1, Words8{});
    for (unsigned l = 0; l < nlevels; l++) {
      unsigned G;
      if (fscanf(f, "%x", &G) != 1 || G == 0 || G > n) return 3;
      std::vector<uint32_t> gates(G);
      for (unsigned s = 0; s < G; s++) {
        unsigned g;
        if (fscanf(f, "%x", &g) != 1 || g >= n || (s && g <= gates[s - 1])) return 5;
        gates[s] = g;
      }
      std::vector<Words8> trip(9 * (size_t)G), opened(2 * (size_t)G), masked[2];
      for (auto &t : trip) if (!read_words(f, &t)) return 4;
      for (auto &o : opened) if (!read_words(f, &o)) return 4;
      for (int form = 0; form < 2; form++) {
        masked[form].assign(6 * (size_t)G, Words8{});
        for (int k = 0; k < 3; k++) {
          const MpcWitPlanes o{P[form][0].data() + k * n, P[form][1].data() + k * n, P[form][2].data() + k * n, vals.data() + k * m,
                               pairs.data() + k * 2 * npairs, chi.data()};
          for (unsigned s = 0; s < G; s++) {
            const uint32_t i = gates[s];
            if (form == 0) {
              mpc_wit_mask_gate(mpc_wit_rows(w, i, k, o), i, 0, k, G, s, o, trip.data(), masked[form].data());
            } else {       // a wave per gate: lane l takes the terms l, l + 64, .. of each row; the reduced parts are added
              const Fn one = mpc_wit_one(k);
              Fn left = fe_zero<FN>(), right = fe_zero<FN>();
              for (uint32_t ln = 0; ln < 64; ln++) {
                left = add(left, fn_reduce(eval_row(w.rows, row_ptr[2 * i] + ln, row_ptr[2 * i + 1], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
                right = add(right, fn_reduce(eval_row(w.rows, row_ptr[2 * i + 1] + ln, row_ptr[2 * i + 2], 64, o.aL, o.aR, o.aO, o.v, one, o.chi)));
              }
              mpc_wit_mask_gate(mpc_wit_pair(op[i], arg[i], left, right, o.inputs), i, 0, k, G, s, o, trip.data(), masked[form].data());
            }
          }
        }
        for (int k = 0; k < 3; k++) {
          const MpcWitPlanes o{P[form][0].data() + k * n, P[form][1].data() + k * n, P[form][2].data() + k * n, vals.data() + k * m,
                               pairs.data() + k * 2 * npairs, chi.data()};
          for (unsigned s = 0; s < G; s++) mpc_wit_combine_gate(gates[s], 0, k, G, s, o, opened.data(), trip.data());
        }
      }
      for (int k = 0; k < 3; k++)
        for (unsigned s = 0; s < G; s++) {
          const size_t i = (size_t)k * n + gates[s];
          for (int form = 0; form < 2; form++) {
            const Words8 *out[5] = {&P[form][0][i], &P[form][1][i], &masked[form][(size_t)k * G + s], &masked[form][(size_t)(3 + k) * G + s],
                                    &P[form][2][i]};
            for (int x = 0; x < 5; x++) { print_words(*out[x]); printf(form == 1 && x == 4 ? "\n" : " "); }
          }
        }
    }
  }
  fclose(f);
  return 0;
}
