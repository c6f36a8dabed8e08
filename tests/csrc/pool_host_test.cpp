// pool_host_test.cpp -- the worker set of bpgpu_pool (mpc_bulletproof_amd/csrc/pool_workers.hpp) on the CPU: 1, 3 and 32 workers
// through 1 000 rounds of fake jobs.  Per round some jobs sleep, one or two fail (one returns an error code or throws; the joined
// error must be the LOWEST failing slot's) and some slots have an empty share (no job: the slot is not woken).  Every job must run
// exactly once per round, on its own slot's thread.  Then the shutdowns: with rounds run, with no round ever run, twice in a row.
// tests/test_pool_workers_cpu.py builds this file twice (-fsanitize=thread and -fsanitize=address,undefined) and runs both binaries:
// the counters below are plain ints on purpose, so that the thread sanitizer checks the ordering that run() promises.
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

#include "pool_workers.hpp"

using bppool::Workers;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { failures++; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static const int THROWN = -77;

static void rounds(size_t n, int nrounds) {
  Workers w(THROWN);
  std::vector<int> started(n, 0);
  std::vector<std::thread::id> tid(n);
  EXPECT(w.start(n, [&](size_t s) { started[s]++; tid[s] = std::this_thread::get_id(); }));
  EXPECT(w.size() == n);
  EXPECT(!w.start(n));                                 // already running
  std::vector<int> ran(n, 0), expect(n, 0), wrong_thread(n, 0);
  std::vector<int> codes;
  for (int r = 0; r < nrounds; r++) {
    const size_t fail = (size_t)(r * 7 + 3) % n;       // one failing slot per round ...
    const size_t fail2 = (r % 3 == 0 && n > 1) ? (size_t)(r * 5 + 1) % n : fail;   // ... and on every third round a second one
    const bool throws = (r & 1) != 0;
    std::vector<Workers::Job> jobs(n);
    size_t lowest = n;
    for (size_t s = 0; s < n; s++) {
      const bool fails = s == fail || s == fail2;
      if (!fails && (s + (size_t)r) % 5 == 4) continue;                            // an empty share
      const bool sleeps = (r % 16 == 0) && (s % 3 == (size_t)r / 16 % 3);
      const int code = fails ? -(int)(s + 1) : 0;
      if (fails && s < lowest) lowest = s;
      expect[s]++;
      jobs[s] = [&, s, sleeps, code, fails, throws]() -> int {
        ran[s]++;
        if (std::this_thread::get_id() != tid[s]) wrong_thread[s]++;
        if (sleeps) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (fails && throws) throw std::runtime_error("job failed");
        return code;
      };
    }
    const long bad = w.run(jobs, codes);
    EXPECT(bad == (long)lowest);
    EXPECT(codes.size() == n);
    for (size_t s = 0; s < n; s++) {
      const bool fails = s == fail || s == fail2;
      EXPECT(codes[s] == (fails ? (throws ? THROWN : -(int)(s + 1)) : 0));
      EXPECT(ran[s] == expect[s]);
    }
  }
  // a round without any job returns at once, and a round after failures is clean
  std::vector<Workers::Job> none(n);
  EXPECT(w.run(none, codes) == -1);
  std::vector<Workers::Job> all(n);
  for (size_t s = 0; s < n; s++) all[s] = [&, s]() -> int { ran[s]++; return 0; };
  EXPECT(w.run(all, codes) == -1);
  for (size_t s = 0; s < n; s++) {
    EXPECT(ran[s] == expect[s] + 1);
    EXPECT(wrong_thread[s] == 0);
  }
  w.stop();
  for (size_t s = 0; s < n; s++) EXPECT(started[s] == 1);
  EXPECT(w.size() == 0);
  w.stop();                                            // a second shutdown is harmless
}

static void never_submitted(size_t n) {
  {
    Workers w(THROWN);
    EXPECT(w.start(n));
  }                                                    // destructor: wakes and joins threads that never had a job
  Workers w(THROWN);                                   // never started at all
  EXPECT(w.size() == 0);
  Workers again(THROWN);                               // start, stop, start: the set is reusable
  EXPECT(again.start(n));
  again.stop();
  EXPECT(again.start(n));
  std::vector<int> codes;
  std::vector<Workers::Job> jobs(n);
  int hits = 0;
  jobs[n - 1] = [&]() -> int { hits++; return 0; };
  EXPECT(again.run(jobs, codes) == -1);
  EXPECT(hits == 1);
}

int main() {
  for (size_t n : {(size_t)1, (size_t)3, (size_t)32}) {
    rounds(n, 1000);
    never_submitted(n);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("all passed\n");
  return 0;
}
