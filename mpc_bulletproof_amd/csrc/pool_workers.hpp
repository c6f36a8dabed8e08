// pool_workers.hpp -- the worker set of a bpgpu_pool (bpgpu_pool.hip): N persistent host threads, one per slot, that run one job per
// slot and round and are joined before run() returns.  No HIP and no project header in here: the set is built and tested on the CPU
// (tests/csrc/pool_host_test.cpp, under the thread and the address sanitizer).
//   Workers w; w.start(n, on_thread_start)   n threads; on_thread_start(slot) runs first on each (the pool selects the slot's device there)
//   w.run(jobs, codes)                       jobs[s] runs on thread s (an empty std::function: slot s is not woken and reports 0); blocks
//                                            until every job of the round has returned; codes[s] = what it returned, or throw_code
//                                            when it threw; returns the lowest slot with a non-zero code, or -1
//   ~Workers / stop()                        wakes and joins the threads; legal with no round ever run
// run() is not re-entrant: the owner serialises its rounds (the pool holds its mutex across a call).
#ifndef BPGPU_POOL_WORKERS_HPP
#define BPGPU_POOL_WORKERS_HPP
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

namespace bppool {

class Workers {
 public:
  using Job = std::function<int()>;
  explicit Workers(int throw_code = -1) : throw_code_(throw_code) {}
  Workers(const Workers &) = delete;
  Workers &operator=(const Workers &) = delete;
  ~Workers() { stop(); }

  // false when a thread cannot be started (those already running are stopped again)
  bool start(size_t n, std::function<void(size_t)> on_thread_start = nullptr) {
    if (!threads_.empty() || !n) return false;
    try {
      slots_.assign(n, Slot{});
      threads_.reserve(n);
      for (size_t s = 0; s < n; s++) threads_.emplace_back([this, s, on_thread_start] { loop(s, on_thread_start); });
    } catch (const std::system_error &) {
      stop();
      return false;
    } catch (const std::bad_alloc &) {
      stop();
      return false;
    }
    return true;
  }
  size_t size() const { return threads_.size(); }

  long run(const std::vector<Job> &jobs, std::vector<int> &codes) {
    const size_t n = threads_.size();
    codes.assign(n, 0);
    {
      std::unique_lock<std::mutex> lk(mu_);
      for (size_t s = 0; s < n && s < jobs.size(); s++)
        if (jobs[s]) { slots_[s].job = &jobs[s]; slots_[s].code = 0; pending_++; }
      if (pending_) {
        wake_.notify_all();
        done_.wait(lk, [this] { return pending_ == 0; });
      }
      for (size_t s = 0; s < n; s++) codes[s] = slots_[s].code, slots_[s].code = 0;
    }
    for (size_t s = 0; s < n; s++)
      if (codes[s]) return (long)s;
    return -1;
  }

  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    wake_.notify_all();
    for (auto &t : threads_)
      if (t.joinable()) t.join();
    threads_.clear();
    slots_.clear();
    quit_ = false;
  }

 private:
  struct Slot { const Job *job = nullptr; int code = 0; };
  void loop(size_t s, const std::function<void(size_t)> &on_thread_start) {
    if (on_thread_start) {
      try { on_thread_start(s); } catch (...) {}
    }
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      wake_.wait(lk, [&] { return quit_ || slots_[s].job; });
      if (!slots_[s].job) return;          // (a job handed over before the shutdown still runs: run() is waiting for it)
      const Job *job = slots_[s].job;
      lk.unlock();
      int code;
      try { code = (*job)(); } catch (...) { code = throw_code_; }
      lk.lock();
      slots_[s].job = nullptr;
      slots_[s].code = code;
      if (--pending_ == 0) done_.notify_all();
    }
  }
  const int throw_code_;
  std::mutex mu_;
  std::condition_variable wake_, done_;
  std::vector<Slot> slots_;
  std::vector<std::thread> threads_;
  size_t pending_ = 0;
  bool quit_ = false;
};

}  // namespace bppool
#endif
