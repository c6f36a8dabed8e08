// queue_plan.h -- the plan of a mixed verifier queue (bpgpu_r1cs_verify_mixed_*, bpgpu_r1cs_verify_mixed_wire_*) and the layout of its
// host forms' staging buffer: host arithmetic only.  No HIP and no project header in here: both are built and tested on the CPU
// (tests/csrc/queue_plan_host_test.cpp, under the address sanitizer).
//   mixed_plan(shapes, ngroups, max_proofs, max_points, max_segs, segs, checks)   which proofs share a check
//   stage_layout(bytes, nfields, off, &total)                                    where one group's fields go in the staging buffer
#ifndef BPGPU_QUEUE_PLAN_H
#define BPGPU_QUEUE_PLAN_H
#include <cstddef>
#include <vector>

namespace bpqueue {

struct QueueShape { size_t nb, nvar; };    // what the plan reads of a group: its proofs, and the proof points of one proof
struct MixSeg { size_t gi, lo, cnt; };     // a run of one group's consecutive proofs
struct MixCheck { size_t first, nseg; };   // a range of the plan's segment list

// The groups' proofs are concatenated (group after group) and cut into checks of at most max_proofs proofs, max_points proof points
// (a single proof may exceed it) and max_segs segments; (size_t)-1 is no budget.
inline void mixed_plan(const QueueShape *G, size_t ngroups, size_t max_proofs, size_t max_points, size_t max_segs,
                       std::vector<MixSeg> &segs, std::vector<MixCheck> &checks) {
  size_t cp = 0, cpts = 0;
  auto close = [&]() { if (!checks.empty() && checks.back().nseg) { checks.push_back(MixCheck{segs.size(), 0}); } cp = cpts = 0; };
  checks.push_back(MixCheck{0, 0});
  for (size_t gi = 0; gi < ngroups; gi++) {
    const size_t nvar = G[gi].nvar;
    size_t lo = 0;
    while (lo < G[gi].nb) {
      if (checks.back().nseg == max_segs) close();
      size_t room = max_proofs - cp, fit = cpts < max_points ? (max_points - cpts) / nvar : 0;
      if (fit < room) room = fit;
      if (!room) {
        if (cp) { close(); continue; }
        room = 1;      // one proof larger than the point budget: a check of its own
      }
      const size_t cnt = G[gi].nb - lo < room ? G[gi].nb - lo : room;
      segs.push_back(MixSeg{gi, lo, cnt});
      checks.back().nseg++;
      cp += cnt; cpts += cnt * nvar; lo += cnt;
      if (cp >= max_proofs || cpts >= max_points) close();
    }
  }
  if (!checks.back().nseg) checks.pop_back();
}

// One group's fields in the staging buffer, one after the other from *total on, each on a 256-byte boundary: off[j] is where field j
// (bytes[j] long; 0 for an absent field, which takes no room) starts, and *total moves past the group.  The sizing pass and the
// upload pass walk the groups with the same calls.
inline void stage_layout(const size_t *bytes, size_t nfields, size_t *off, size_t *total) {
  for (size_t j = 0; j < nfields; j++) {
    off[j] = *total;
    *total += (bytes[j] + 255) / 256 * 256;
  }
}

}  // namespace bpqueue
#endif
