// CPU build (g++ -fsanitize=undefined) of the row evaluation of fn_dev.cuh (eval_row: one constraint row against one prover's
// witness), driven as k_rows_eval drives it: the whole row by one lane, and the row spread over 64 lanes whose reduced parts are
// added up.  Reads cases from a file, prints one line of residuals per case.  Test infrastructure only.
//
// Case file, integers as hex: `ncases`, then per case `nterms nvals nchi one`, the nchi gadget challenges, the nvals values (all
// plain canonical), and nterms terms `kind idx j coeff` (kind 0..3 read values[idx], kind 4 is the constant; coeff plain canonical).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/fn_dev.cuh"
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
void print_fn(const Fn &x) {
  uint32_t w[8];
  pack(w, from_mont(x));
  for (int j = 7; j >= 0; j--) printf("%08x", w[j]);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned ncases = 0;
  if (fscanf(f, "%x", &ncases) != 1) return 3;
  for (unsigned c = 0; c < ncases; c++) {
    unsigned nterms, nvals, nchi, one_flag;
    if (fscanf(f, "%x %x %x %x", &nterms, &nvals, &nchi, &one_flag) != 4) return 3;
    std::vector<Words8> chi(nchi ? nchi : 1), vals(nvals ? nvals : 1), coeff(nterms ? nterms : 1);
    std::vector<uint32_t> var(nterms ? nterms : 1);
    for (unsigned i = 0; i < nchi; i++) if (!read_words(f, &chi[i])) return 4;
    for (unsigned i = 0; i < nvals; i++) if (!read_words(f, &vals[i])) return 4;
    for (unsigned t = 0; t < nterms; t++) {
      unsigned kind, idx, j;
      Words8 cw;
      if (fscanf(f, "%x %x %x", &kind, &idx, &j) != 3 || !read_words(f, &cw)) return 4;
      if (kind > 4 || (kind < 4 && idx >= nvals) || j > nchi) return 5;
      var[t] = idx | kind << ROWS_KIND_SHIFT | j << ROWS_CHI_SHIFT;
      pack(coeff[t].w, canon(to_mont(unpack<FN>(cw.w))));          // the handle keeps coefficients in Montgomery form
    }
    RowsDev rv{};
    rv.var = var.data(); rv.coeff = coeff.data(); rv.q = 1; rv.nnz = nterms;
    const Fn one = one_flag ? fe_one<FN>() : fe_zero<FN>();
    const Words8 *v = vals.data();
    // a lane per row
    const Fn lane = fn_reduce(eval_row(rv, 0, nterms, 1, v, v, v, v, one, chi.data()));
    // a wave per row: lane l takes the terms l, l + 64, ..; the reduced parts are added, then reduced once more
    Fn wave = fe_zero<FN>();
    for (uint32_t l = 0; l < 64; l++) wave = add(wave, fn_reduce(eval_row(rv, l, nterms, 64, v, v, v, v, one, chi.data())));
    print_fn(lane);
    printf(" ");
    print_fn(fn_reduce(wave));
    printf("\n");
  }
  fclose(f);
  return 0;
}
