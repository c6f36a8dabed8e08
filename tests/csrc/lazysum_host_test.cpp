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
Fn pow_u32(Fn base, uint32_t e) {   // fn_pow_u32 of fn_dev.cuh (device only there)
  Fn acc = fe_one<FN>();
  while (e) {
    if (e & 1) acc = mul(acc, base);
    e >>= 1;
    if (e) base = sqr(base);
  }
  return acc;
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
      const Fn yi = pow_u32(y, i);
      const Fn l = add(aL, mul(pow_u32(y, i), zero)), r0 = sub(zero, yi), r1 = add(mul(yi, aR), zero);
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
