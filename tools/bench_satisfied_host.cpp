// The host mirror's Prover::constraints_satisfied() loop (mpc_bulletproof_amd/host/mpc_bulletproof.cpp) over nb provers that each
// range-prove nvals values of n_bits bits in one constraint system: what bpgpu_r1cs_constraints_satisfied replaces.  Built and run by
// tools/bench_satisfied.py; prints the wall clock of each repetition in ms.  No device call: the commitments are placeholders.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "gadgets.hpp"

using namespace mpc_bulletproof;
using namespace mpc_bulletproof::r1cs;

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const size_t nb = strtoul(argv[1], nullptr, 10), nvals = strtoul(argv[2], nullptr, 10), n_bits = strtoul(argv[3], nullptr, 10),
               reps = strtoul(argv[4], nullptr, 10);
  PedersenGens pc_gens;
  std::vector<std::unique_ptr<Transcript>> trs;
  std::vector<std::unique_ptr<Prover>> provers;
  for (size_t p = 0; p < nb; p++) {
    trs.emplace_back(new Transcript("RangeProofTest"));
    provers.emplace_back(new Prover(pc_gens, *trs.back()));
    for (size_t j = 0; j < nvals; j++) {
      uint64_t v = 0x9E3779B97F4A7C15ull * (j + 1 + 31 * p);
      if (n_bits < 64) v &= (1ull << n_bits) - 1;
      Variable var = provers[p]->commit_precomputed(Scalar::from(v), Scalar::from((uint64_t)1), StarkPoint::generator());
      gadgets::range_proof(*provers[p], LinearCombination(var), &v, n_bits);
    }
  }
  for (size_t r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    size_t good = 0;
    for (auto &pv : provers) good += pv->constraints_satisfied() ? 1 : 0;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (good != nb) return 3;
    printf("MS %.3f\n", ms);
  }
  return 0;
}
