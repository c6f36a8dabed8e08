// CPU build (g++ -fsanitize=undefined) of the lazy F_n sums of the scalar kernels, restated with the BP_HD helpers of fe29.cuh and
// fn_dev.cuh alone: a lane adds unreduced Montgomery products and folds them with fn_reduce every `fold` trips, the lanes' reduced
// sums go through a 64-way butterfly in wave_sum's order, the four waves are added, and store_plain or fn_reduce ends the sum.  A
// signed overflow anywhere ends the program (-fno-sanitize-recover).  Reads commands from a file, prints one line per command.  Test
// infrastructure only.
//
// Commands, integers as hex, scalars plain canonical:
//   raw a b                 the limbs of mul(load_plain(a), load_plain(b)), decimal, least significant first
//   rawload a               the limbs of load_plain(a) (a Beaver term's z)
//   plane aL aR y i         the limbs of l * r0 and of l * r1 as k_prover_polys stores the planes at index i for vanishing weights:
//                           l = load_plain(aL), r0 = 0 - y^i, r1 = y^i * load_plain(aR)
//   block fold final L nt plen, then plen * nt terms `kind a b`
//                           a block of 256 lanes over L elements (stride 256), nt terms per element, element i reading pattern entry
//                           i mod plen; term kinds: 0 a * b, 1 a * (0 - b) (a lazily negative factor), 2 load_plain(a) alone;
//                           final 0: store_plain of the four waves' sum, 1: fn_reduce of it first (a partial of inner_product)
//   ip grid fold L plen, then plen pairs `a b`
//                           k_inner_product_partial over `grid` blocks and k_inner_product_finish over their partials
//   finish nparts plen, then plen pairs `a b`
//                           k_inner_product_finish over nparts partials, partial i = fn_reduce(a * b) of pattern entry i mod plen
// The verifier's sites (every term list is plen terms `kind a b` as for `block`; element i reads term i mod plen):
//   wave pre fold L plen, terms
//                           one wave of 64 lanes over L elements (stride 64), one term each: k_verify_scalars' `One`-column loop
//                           (pre 0: add, then fold) and its delta loop (pre 1: fold at the head of the trip, then add); fn_reduce,
//                           the butterfly, fn_reduce, store_plain of the NEGATED sum (w_c's sign; delta's shape is the same up to it)
//   column fold E negate mult plen, terms
//                           flatten_column over E entries, serial, the lazy result negated (a V column) or not and multiplied by
//                           load_plain(mult): V_j = w_V,j r x^2
//   hexpr fold E x yi b sr plen, terms of the L column, terms of the O column
//                           h_i = yi (x wL + wO - b sr) - 1 on two lazy columns of E entries each, and on the same line
//                           g-side delta term (wO yi) wL: the two places a lazy column meets another product
//   tail fold nparts waves plen, terms
//                           k_vsl_tail: nparts partials, partial i the unreduced sum of `waves` reduced terms, added with a fold
//                           after every fold-th; fn_reduce; negated
//   mix fold nseg len_1 .. len_nseg plen, terms
//                           mix_colsum_body: 256 lanes over nseg segments, ONE counter per lane across them; a single segment is
//                           k_sc_weighted_colsum / comb_colsum_body
//   split pre fold tfold grid L plen, terms
//                           k_vsl_wc (pre 0) / k_vsl_gh (pre 1: fold at the head of the trip): `grid` blocks of 128 lanes over L
//                           elements (stride grid * 128), fold in the loop, two waves per block, then k_vsl_tail's sum of the grid
//                           partials with fold tfold; negated
//   sumraw count a b        fn_reduce of `count` unreduced products a * b added up, then the canonical value
//   sumred count a b        `count` reduced products fn_reduce(a * b) added up, then the canonical value with no reduction between
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../mpc_bulletproof_amd/csrc/fn_dev.cuh"
using namespace bp;
using namespace bpk;

namespace {
constexpr int TPB = 256;

bool read_words(FILE *f, Words8 *out) {
  char s[80];
  if (fscanf(f, "%79s", s) != 1) return false;
  std::string h(s);
  if (h.size() > 64) return false;
  h = std::string(64 - h.size(), '0') + h;
  for (int j = 0; j < 8; j++) out->w[j] = (uint32_t)strtoul(h.substr(64 - 8 * (j + 1), 8).c_str(), nullptr, 16);
  return words_lt_mod<FN>(out->w);
}
bool read_fn(FILE *f, Fn *out) {
  Words8 w;
  if (!read_words(f, &w)) return false;
  *out = load_plain(&w);
  return true;
}
void print_plain(const Fn &x) {   // store_plain's conversion
  uint32_t w[8];
  pack(w, from_mont(x));
  for (int j = 7; j >= 0; j--) printf("%08x", w[j]);
}
void print_limbs(const Fn &x) {
  for (int j = 0; j < NL; j++) printf("%s%d", j ? "," : "", x.v[j]);
}
// wave_sum's butterfly over the 64 lanes of one wave: every lane adds its partner's value, off = 32, 16, .., 1
Fn wave_sum_host(Fn *x) {
  for (int off = 32; off > 0; off >>= 1) {
    Fn y[64];
    for (int l = 0; l < 64; l++) y[l] = add(x[l], x[l ^ off]);
    for (int l = 0; l < 64; l++) x[l] = y[l];
  }
  return x[0];
}
// the block tail every site shares: fn_reduce per lane, wave_sum per wave, the waves added by lane 0
Fn block_tail(std::vector<Fn> &lanes) {
  for (auto &x : lanes) x = fn_reduce(x);
  Fn t = wave_sum_host(lanes.data());
  for (int w = 1; w < TPB / 64; w++) t = add(t, wave_sum_host(lanes.data() + 64 * w));
  return t;
}
Fn finish(const std::vector<Fn> &partials) {
  std::vector<Fn> lanes(64, fe_zero<FN>());
  for (int l = 0; l < 64; l++)
    for (size_t i = l; i < partials.size(); i += 64) lanes[l] = add(lanes[l], partials[i]);
  for (auto &x : lanes) x = fn_reduce(x);
  return wave_sum_host(lanes.data());
}
// a term list: kind 0 a * b, 1 a * (0 - b), 2 load_plain(a) alone
bool read_terms(FILE *f, size_t count, std::vector<Fn> *out) {
  const Fn zero = fe_zero<FN>();
  out->resize(count);
  for (auto &t : *out) {
    unsigned kind;
    Fn a, b;
    if (fscanf(f, "%x", &kind) != 1 || kind > 2 || !read_fn(f, &a) || !read_fn(f, &b)) return false;
    t = kind == 0 ? mul(a, b) : (kind == 1 ? mul(a, sub(zero, b)) : a);
  }
  return true;
}
// flatten_column's loop over E entries
Fn column(const std::vector<Fn> &terms, unsigned E, unsigned fold) {
  Fn acc = fe_zero<FN>();
  unsigned cnt = 0;
  for (unsigned t = 0; t < E; t++) {
    acc = add(acc, terms[t % terms.size()]);
    if (++cnt % fold == 0) acc = fn_reduce(acc);
  }
  return acc;
}
// k_vsl_tail's sum of partials
Fn tail_sum(const std::vector<Fn> &parts, unsigned fold) {
  Fn acc = fe_zero<FN>();
  for (size_t i = 0; i < parts.size(); i++) {
    acc = add(acc, parts[i]);
    if (i % fold == fold - 1) acc = fn_reduce(acc);
  }
  return fn_reduce(acc);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  const Fn zero = fe_zero<FN>();
  while (fscanf(f, "%15s", cmd) == 1) {
    const std::string c(cmd);
    if (c == "raw") {
      Fn a, b;
      if (!read_fn(f, &a) || !read_fn(f, &b)) return 4;
      print_limbs(mul(a, b));
    } else if (c == "rawload") {
      Fn a;
      if (!read_fn(f, &a)) return 4;
      print_limbs(a);
    } else if (c == "plane") {
      Fn aL, aR, y;
      unsigned i;
      if (!read_fn(f, &aL) || !read_fn(f, &aR) || !read_fn(f, &y) || fscanf(f, "%x", &i) != 1) return 4;
      const Fn yi = fn_pow_u32(y, i);
      const Fn l = add(aL, mul(fn_pow_u32(y, i), zero)), r0 = sub(zero, yi), r1 = add(mul(yi, aR), zero);
      print_limbs(mul(l, r0));
      printf(" ");
      print_limbs(mul(l, r1));
    } else if (c == "block") {
      unsigned fold, fin, L, nt, plen;
      if (fscanf(f, "%x %x %x %x %x", &fold, &fin, &L, &nt, &plen) != 5 || !fold || !nt || !plen || fin > 1) return 3;
      std::vector<Fn> terms((size_t)plen * nt);
      for (auto &t : terms) {
        unsigned kind;
        Fn a, b;
        if (fscanf(f, "%x", &kind) != 1 || kind > 2 || !read_fn(f, &a) || !read_fn(f, &b)) return 4;
        t = kind == 0 ? mul(a, b) : (kind == 1 ? mul(a, sub(zero, b)) : a);
      }
      std::vector<Fn> lanes(TPB, zero);
      for (unsigned t = 0; t < TPB; t++) {
        Fn acc = zero;
        unsigned cnt = 0;
        for (unsigned i = t; i < L; i += TPB) {
          for (unsigned j = 0; j < nt; j++) acc = add(acc, terms[(size_t)(i % plen) * nt + j]);
          if (++cnt % fold == 0) acc = fn_reduce(acc);
        }
        lanes[t] = acc;
      }
      const Fn t = block_tail(lanes);
      print_plain(fin ? fn_reduce(t) : t);
    } else if (c == "ip") {
      unsigned grid, fold, L, plen;
      if (fscanf(f, "%x %x %x %x", &grid, &fold, &L, &plen) != 4 || !grid || !fold || !plen) return 3;
      std::vector<Fn> terms(plen);
      for (auto &t : terms) {
        Fn a, b;
        if (!read_fn(f, &a) || !read_fn(f, &b)) return 4;
        t = mul(a, b);
      }
      std::vector<Fn> partials(grid);
      for (unsigned blk = 0; blk < grid; blk++) {
        std::vector<Fn> lanes(TPB, zero);
        for (unsigned t = 0; t < TPB; t++) {
          Fn acc = zero;
          unsigned cnt = 0;
          for (size_t i = (size_t)blk * TPB + t; i < L; i += (size_t)grid * TPB) {
            acc = add(acc, terms[i % plen]);
            if (++cnt % fold == 0) acc = fn_reduce(acc);
          }
          lanes[t] = acc;
        }
        partials[blk] = fn_reduce(block_tail(lanes));
      }
      print_plain(finish(partials));
    } else if (c == "finish") {
      unsigned nparts, plen;
      if (fscanf(f, "%x %x", &nparts, &plen) != 2 || !plen) return 3;
      std::vector<Fn> terms(plen);
      for (auto &t : terms) {
        Fn a, b;
        if (!read_fn(f, &a) || !read_fn(f, &b)) return 4;
        t = fn_reduce(mul(a, b));
      }
      std::vector<Fn> partials(nparts);
      for (unsigned i = 0; i < nparts; i++) partials[i] = terms[i % plen];
      print_plain(finish(partials));
    } else if (c == "wave") {
      unsigned pre, fold, L, plen;
      std::vector<Fn> terms;
      if (fscanf(f, "%x %x %x %x", &pre, &fold, &L, &plen) != 4 || pre > 1 || !fold || !plen || !read_terms(f, plen, &terms)) return 3;
      Fn lanes[64];
      for (unsigned t = 0; t < 64; t++) {
        Fn acc = zero;
        unsigned cnt = 0;
        for (unsigned i = t; i < L; i += 64) {
          if (pre && ++cnt % fold == 0) acc = fn_reduce(acc);
          acc = add(acc, terms[i % plen]);
          if (!pre && ++cnt % fold == 0) acc = fn_reduce(acc);
        }
        lanes[t] = fn_reduce(acc);
      }
      print_plain(neg(fn_reduce(wave_sum_host(lanes))));
    } else if (c == "column") {
      unsigned fold, E, negate, plen;
      Fn mult;
      std::vector<Fn> terms;
      if (fscanf(f, "%x %x %x", &fold, &E, &negate) != 3 || !fold || negate > 1 || !read_fn(f, &mult) || fscanf(f, "%x", &plen) != 1 || !plen ||
          !read_terms(f, plen, &terms))
        return 3;
      Fn acc = column(terms, E, fold);
      if (negate) acc = neg(acc);
      print_plain(mul(acc, mult));
    } else if (c == "hexpr") {
      unsigned fold, E, plen;
      Fn x, yi, b, sr;
      std::vector<Fn> tl, to;
      if (fscanf(f, "%x %x", &fold, &E) != 2 || !fold || !read_fn(f, &x) || !read_fn(f, &yi) || !read_fn(f, &b) || !read_fn(f, &sr) ||
          fscanf(f, "%x", &plen) != 1 || !plen || !read_terms(f, plen, &tl) || !read_terms(f, plen, &to))
        return 3;
      const Fn wL = column(tl, E, fold), wO = column(to, E, fold);
      print_plain(sub(mul(yi, sub(add(mul(x, wL), wO), mul(b, sr))), fe_one<FN>()));
      printf(" ");
      print_plain(mul(mul(wO, yi), wL));
    } else if (c == "tail") {
      unsigned fold, nparts, waves, plen;
      std::vector<Fn> terms;
      if (fscanf(f, "%x %x %x %x", &fold, &nparts, &waves, &plen) != 4 || !fold || !waves || !plen || !read_terms(f, plen, &terms)) return 3;
      std::vector<Fn> parts(nparts);
      for (unsigned i = 0; i < nparts; i++) {
        Fn t = fn_reduce(terms[(size_t)i * waves % plen]);
        for (unsigned w = 1; w < waves; w++) t = add(t, fn_reduce(terms[((size_t)i * waves + w) % plen]));
        parts[i] = t;
      }
      print_plain(neg(tail_sum(parts, fold)));
    } else if (c == "mix") {
      unsigned fold, nseg, plen;
      if (fscanf(f, "%x %x", &fold, &nseg) != 2 || !fold || !nseg || nseg > 16) return 3;
      std::vector<unsigned> len(nseg);
      for (auto &l : len)
        if (fscanf(f, "%x", &l) != 1) return 3;
      std::vector<Fn> terms;
      if (fscanf(f, "%x", &plen) != 1 || !plen || !read_terms(f, plen, &terms)) return 3;
      std::vector<Fn> lanes(TPB, zero);
      for (unsigned t = 0; t < TPB; t++) {
        Fn acc = zero;
        unsigned cnt = 0;
        size_t base = 0;
        for (unsigned s = 0; s < nseg; s++) {
          for (unsigned p = t; p < len[s]; p += TPB) {
            acc = add(acc, terms[(base + p) % plen]);
            if (++cnt % fold == 0) acc = fn_reduce(acc);
          }
          base += len[s];
        }
        lanes[t] = acc;
      }
      print_plain(block_tail(lanes));
    } else if (c == "split") {
      unsigned pre, fold, tfold, grid, L, plen;
      std::vector<Fn> terms;
      if (fscanf(f, "%x %x %x %x %x %x", &pre, &fold, &tfold, &grid, &L, &plen) != 6 || pre > 1 || !fold || !tfold || !grid || grid > 256 || !plen ||
          !read_terms(f, plen, &terms))
        return 3;
      std::vector<Fn> parts(grid);
      for (unsigned blk = 0; blk < grid; blk++) {
        Fn lanes[128];
        for (unsigned t = 0; t < 128; t++) {
          Fn acc = zero;
          unsigned cnt = 0;
          for (size_t i = (size_t)blk * 128 + t; i < L; i += (size_t)grid * 128) {
            if (pre && ++cnt % fold == 0) acc = fn_reduce(acc);
            acc = add(acc, terms[i % plen]);
            if (!pre && ++cnt % fold == 0) acc = fn_reduce(acc);
          }
          lanes[t] = fn_reduce(acc);
        }
        parts[blk] = add(fn_reduce(wave_sum_host(lanes)), fn_reduce(wave_sum_host(lanes + 64)));
      }
      print_plain(neg(tail_sum(parts, tfold)));
    } else if (c == "sumraw" || c == "sumred") {
      unsigned count;
      Fn a, b;
      if (fscanf(f, "%x", &count) != 1 || !read_fn(f, &a) || !read_fn(f, &b)) return 4;
      const bool red = c == "sumred";
      const Fn t = red ? fn_reduce(mul(a, b)) : mul(a, b);
      Fn acc = zero;
      for (unsigned i = 0; i < count; i++) acc = add(acc, t);
      print_plain(red ? acc : fn_reduce(acc));
    } else {
      return 3;
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
