// queue_plan_host_test.cpp -- the plan of the mixed verifier queues and their staging layout (mpc_bulletproof_amd/csrc/queue_plan.h)
// on the CPU: crafted queues against recorded plans, 120 000 random queues against the plan's invariants, and the layout's rules.
// A stand-alone program: tests/test_queue_plan_cpu.py builds it with the host compiler under the address and undefined-behaviour
// sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "queue_plan.h"

using namespace bpqueue;

static const size_t U = (size_t)-1, CAP = 16;
static int failures = 0;
#define EXPECT(cond, ...)                                         \
  do {                                                            \
    if (!(cond)) {                                                \
      if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                             \
  } while (0)

static std::string plan_text(const std::vector<MixSeg> &segs, const std::vector<MixCheck> &checks) {
  std::string s;
  for (size_t c = 0; c < checks.size(); c++) {
    s += c ? " [" : "[";
    for (size_t i = 0; i < checks[c].nseg; i++) {
      const MixSeg &g = segs[checks[c].first + i];
      s += "(" + std::to_string(g.gi) + "," + std::to_string(g.lo) + "," + std::to_string(g.cnt) + ")";
    }
    s += "]";
  }
  return s;
}
static void crafted(const char *name, const std::vector<QueueShape> &G, size_t max_proofs, size_t max_points, const std::string &want) {
  std::vector<MixSeg> segs;
  std::vector<MixCheck> checks;
  mixed_plan(G.data(), G.size(), max_proofs, max_points, CAP, segs, checks);
  const std::string got = plan_text(segs, checks);
  EXPECT(got == want, "%s: got '%s', expected '%s'", name, got.c_str(), want.c_str());
}
static void crafted_queues() {
  crafted("one group, proof budget", {{5, 18}}, 4, U, "[(0,0,4)] [(0,4,1)]");
  crafted("one group, point budget", {{10, 18}}, 100, 64, "[(0,0,3)] [(0,3,3)] [(0,6,3)] [(0,9,1)]");
  crafted("each proof exceeds the point budget", {{2, 100}}, 100, 64, "[(0,0,1)] [(0,1,1)]");
  crafted("a check over two groups", {{2, 18}, {3, 18}}, 4, U, "[(0,0,2)(1,0,2)] [(1,2,1)]");
  crafted("empty groups around one", {{0, 18}, {2, 18}, {0, 18}}, 4, U, "[(1,0,2)]");
  {
    std::string want = "[";
    for (int g = 0; g < 16; g++) want += "(" + std::to_string(g) + ",0,1)";
    want += "] [(16,0,1)]";
    crafted("the segment cap", std::vector<QueueShape>(17, QueueShape{1, 18}), U, U, want);
  }
  crafted("only empty groups", {{0, 18}, {0, 30}}, 4, 64, "");
  crafted("point budget over two circuits", {{3, 18}, {2, 30}}, 100, 90, "[(0,0,3)(1,0,1)] [(1,1,1)]");
  crafted("both budgets reached at once", {{4, 18}}, 4, 72, "[(0,0,4)]");
  crafted("no group", {}, 4, 64, "");
}

static void check_invariants(const std::vector<QueueShape> &G, size_t max_proofs, size_t max_points, const std::vector<MixSeg> &segs,
                             const std::vector<MixCheck> &checks, unsigned long q) {
  // the segments in order cover every group's [0, nb) exactly once, group-major; none is empty
  size_t gi = 0, lo = 0;
  for (size_t i = 0; i < segs.size(); i++) {
    const MixSeg &s = segs[i];
    EXPECT(s.gi < G.size() && s.gi >= gi, "queue %lu: segment %zu names group %zu after %zu", q, i, s.gi, gi);
    if (s.gi >= G.size() || s.gi < gi) return;
    while (gi < s.gi) { EXPECT(lo == G[gi].nb, "queue %lu: group %zu left at %zu of %zu", q, gi, lo, G[gi].nb); gi++; lo = 0; }
    EXPECT(s.cnt > 0, "queue %lu: segment %zu is empty", q, i);
    EXPECT(s.lo == lo && s.cnt <= G[gi].nb - lo, "queue %lu: segment %zu = (%zu,%zu,%zu), group at %zu of %zu", q, i, s.gi, s.lo, s.cnt, lo, G[gi].nb);
    lo = s.lo + s.cnt;
  }
  for (; gi < G.size(); gi++, lo = 0) EXPECT(lo == G[gi].nb, "queue %lu: group %zu left at %zu of %zu", q, gi, lo, G[gi].nb);
  // the checks tile the segment list, 1 to 16 segments each
  size_t at = 0;
  for (size_t c = 0; c < checks.size(); c++) {
    EXPECT(checks[c].first == at, "queue %lu: check %zu starts at %zu, not %zu", q, c, checks[c].first, at);
    EXPECT(checks[c].nseg >= 1 && checks[c].nseg <= CAP, "queue %lu: check %zu has %zu segments", q, c, checks[c].nseg);
    at = checks[c].first + checks[c].nseg;
    if (at > segs.size()) break;
  }
  EXPECT(at == segs.size(), "queue %lu: the checks end at segment %zu of %zu", q, at, segs.size());
  if (at != segs.size()) return;
  for (size_t c = 0; c < checks.size(); c++) {
    const MixSeg *sg = segs.data() + checks[c].first;
    const size_t ns = checks[c].nseg;
    size_t proofs = 0, points = 0;
    for (size_t i = 0; i < ns; i++) {
      if (i) EXPECT(sg[i].gi > sg[i - 1].gi, "queue %lu: check %zu: group %zu follows %zu", q, c, sg[i].gi, sg[i - 1].gi);
      proofs += sg[i].cnt;
      points += sg[i].cnt * G[sg[i].gi].nvar;
    }
    EXPECT(proofs <= max_proofs, "queue %lu: check %zu holds %zu proofs of %zu", q, c, proofs, max_proofs);
    EXPECT(points <= max_points || (ns == 1 && sg[0].cnt == 1), "queue %lu: check %zu holds %zu points of %zu", q, c, points, max_points);
    if (c + 1 == checks.size()) continue;
    // ... and could not have taken the first proof of its successor
    const MixSeg &next = segs[checks[c + 1].first];
    const size_t nvar = G[next.gi].nvar;
    const bool full = proofs == max_proofs, no_room = points > max_points || max_points - points < nvar,
               capped = ns == CAP && next.gi != sg[ns - 1].gi;
    EXPECT(full || no_room || capped, "queue %lu: check %zu (%zu proofs, %zu points, %zu segments) stops short of a proof of %zu points", q, c,
           proofs, points, ns, nvar);
  }
}
static void random_queues(unsigned long count) {
  std::mt19937_64 rng(20240607);
  auto below = [&](size_t n) { return (size_t)(rng() % n); };
  for (unsigned long q = 0; q < count && failures < 20; q++) {
    std::vector<QueueShape> G(below(40));
    for (QueueShape &x : G) x = QueueShape{below(4) == 0 ? 0 : below(50), 11 + below(200)};
    const size_t max_proofs = below(2) ? U : 1 + below(64), max_points = below(2) ? U : 1 + below(4000);
    std::vector<MixSeg> segs;
    std::vector<MixCheck> checks;
    mixed_plan(G.data(), G.size(), max_proofs, max_points, CAP, segs, checks);
    check_invariants(G, max_proofs, max_points, segs, checks, q);
  }
}

static void staging_layout() {
  std::mt19937_64 rng(7);
  for (int round = 0; round < 2000 && failures < 20; round++) {
    const size_t ngroups = 1 + rng() % 8, nf = 1 + rng() % 6;
    std::vector<std::vector<size_t>> bytes(ngroups, std::vector<size_t>(nf));
    for (auto &b : bytes) for (size_t &x : b) x = rng() % 3 == 0 ? 0 : 1 + rng() % 5000;
    std::vector<std::vector<size_t>> off[2] = {bytes, bytes};
    size_t total[2] = {0, 0};
    for (int pass = 0; pass < 2; pass++)
      for (size_t i = 0; i < ngroups; i++) stage_layout(bytes[i].data(), nf, off[pass][i].data(), &total[pass]);
    EXPECT(total[0] == total[1] && off[0] == off[1], "round %d: two passes differ", round);
    size_t end = 0;    // of the field before, rounded up
    for (size_t i = 0; i < ngroups; i++)
      for (size_t j = 0; j < nf; j++) {
        const size_t o = off[0][i][j];
        EXPECT(o % 256 == 0, "round %d: offset %zu", round, o);
        EXPECT(o == end, "round %d: group %zu field %zu at %zu, the one before ends at %zu", round, i, j, o, end);   // no overlap, no gap
        end = o + (bytes[i][j] + 255) / 256 * 256;
        if (!bytes[i][j]) EXPECT(end == o, "round %d: an absent field takes room", round);
        EXPECT(end - (o + bytes[i][j]) < 256, "round %d: field of %zu bytes takes %zu", round, bytes[i][j], end - o);
      }
    EXPECT(total[0] == end, "round %d: total %zu, last field ends at %zu", round, total[0], end);
  }
  // a group of the decoded queue by hand: points, scalars, challenges, no gadget challenges, weights, verdicts
  const size_t b[6] = {3 * 18 * 64, 3 * 160, 3 * 7 * 32, 0, 3 * 32, 3 * 4};
  size_t off[6], total = 512;
  stage_layout(b, 6, off, &total);
  const size_t want[6] = {512, 512 + 3584, 512 + 3584 + 512, 512 + 3584 + 512 + 768, 512 + 3584 + 512 + 768, 512 + 3584 + 512 + 768 + 256};
  for (int j = 0; j < 6; j++) EXPECT(off[j] == want[j], "field %d at %zu, expected %zu", j, off[j], want[j]);
  EXPECT(total == want[5] + 256, "total %zu", total);
}

int main() {
  crafted_queues();
  random_queues(120000);
  staging_layout();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("all passed\n");
  return 0;
}
