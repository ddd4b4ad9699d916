// One process-wide pool of worker threads shared by every pool_for, so concurrent
// batch resolutions (tsg_batch_submit pipelines them) never run more than the pool's
// threads plus their callers, and per-thread caches (the backtracker's visited rows)
// survive from one batch to the next.
#include "pool.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace tsg {
namespace {

struct PJob {
  std::function<void(size_t)> body;
  size_t n = 0, grain = 64;
  std::atomic<size_t> next{0};
  int pending = 0;  // queued or running helper tasks (under m)
  std::mutex m;
  std::condition_variable cv;
  void work() {
    for (;;) {
      const size_t s = next.fetch_add(grain);
      if (s >= n) break;
      const size_t e = std::min(n, s + grain);
      for (size_t i = s; i < e; i++) body(i);
    }
  }
};

class Pool {
 public:
  static Pool& get() {
    static Pool* p = new Pool;  // never destroyed: workers may still wait at exit
    return *p;
  }
  // runs j on the caller and up to `helpers` pool threads; returns when all are done
  // at least n worker threads (more concurrent jobs can then run side by side)
  void reserve(int n) { grow(std::min(n, 256)); }
  void run(PJob& j, int helpers) {
    grow(helpers);
    {
      std::lock_guard<std::mutex> g(m_);
      j.pending = helpers;
      for (int h = 0; h < helpers; h++) q_.push_back(&j);
    }
    cv_.notify_all();
    j.work();
    {  // helpers that have not started are not needed any more
      std::lock_guard<std::mutex> g(m_);
      int removed = 0;
      for (auto it = q_.begin(); it != q_.end();)
        if (*it == &j) {
          it = q_.erase(it);
          removed++;
        } else {
          ++it;
        }
      std::lock_guard<std::mutex> g2(j.m);
      j.pending -= removed;
    }
    std::unique_lock<std::mutex> lk(j.m);
    j.cv.wait(lk, [&] { return j.pending == 0; });
  }

 private:
  void grow(int want) {
    std::lock_guard<std::mutex> g(m_);
    while ((int)th_.size() < want) {
      th_.emplace_back([this] { worker(); });
      th_.back().detach();
    }
  }
  void worker() {
    for (;;) {
      PJob* j;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !q_.empty(); });
        j = q_.front();
        q_.pop_front();
      }
      j->work();
      std::lock_guard<std::mutex> g(j->m);
      if (--j->pending == 0) j->cv.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<PJob*> q_;
  std::vector<std::thread> th_;
};

}  // namespace

void pool_reserve(int threads) { Pool::get().reserve(threads); }

void pool_for(size_t n, int nthreads, const std::function<void(size_t)>& f, size_t grain) {
  if (nthreads <= 1 || n < 2 * grain) {
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  PJob j;
  j.body = f;
  j.n = n;
  j.grain = grain;
  Pool::get().run(j, std::min(nthreads, 256) - 1);
}

}  // namespace tsg
