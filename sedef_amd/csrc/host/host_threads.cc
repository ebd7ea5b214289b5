// The host threads of the stage: one pool for the whole process (parallel_for), the lanes of a driver (run_lanes).
// The per-pair host work (anchors, chaining, refinement, CIGAR algebra) is independent across pairs: run it on
// all host cores (SDF_HOST_THREADS overrides).  The reference runs one single-threaded process per bucket.
#include <condition_variable>

#include "stage_internal.h"

namespace sdfh {

void FirstError::set() {
  std::string msg;
  try {
    throw;
  } catch (std::string &s) {
    msg = s.empty() ? std::string("error") : s;
  } catch (std::exception &e) {
    msg = e.what();
  } catch (...) {
    msg = "unknown error";
  }
  std::lock_guard<std::mutex> g(mu_);
  if (!failed_) msg_ = msg;
  failed_ = true;
}

void parallel_for(int n, const std::function<void(int)> &body) {
  const int nthreads = [] {
    const int asked = stage_settings().host_threads;
    int t = asked > 0 ? asked : (int)std::thread::hardware_concurrency();
    if (asked <= 0) {  // a container's CPU quota (cgroup v2 cpu.max = "<quota> <period>") counts, not the host's core count
      if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        long long quota = 0, period = 0;
        if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
          t = std::min<long long>(t, std::max<long long>(1, (quota + period - 1) / period));
        fclose(f);
      }
    }
    return t < 1 ? 1 : (t > 64 ? 64 : t);
  }();
  const int nt = std::min(nthreads, n);
  if (nt <= 1) {
    for (int i = 0; i < n; i++) body(i);
    return;
  }
  // The lanes of the stage driver call this concurrently, a few hundred times per run.  One set of worker threads for
  // the whole process (as many as the CPU quota: more runnable threads get the process throttled) serves all callers:
  // a call is a REGION -- a counter over its items -- queued for the workers; the caller works on its own region too,
  // so it never waits for a parked thread to wake up, and returns when all its items are done.  (Threads created and
  // joined per call cost 0.1 ms each, milliseconds under a CPU quota.)
  struct Region {
    const std::function<void(int)> *body;
    int n;
    std::atomic<int> next{0}, done{0};
    FirstError error;
    void run() {
      for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
        try {
          (*body)(i);
        } catch (...) {
          error.set();
        }
        if (done.fetch_add(1) + 1 == n) {  // the last item: wake the caller if it is waiting
          std::lock_guard<std::mutex> g(fin_mu);
          fin_cv.notify_all();
        }
      }
    }
    std::mutex fin_mu;
    std::condition_variable fin_cv;
  };
  struct Pool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<Region>> open;  // regions that may still have items to hand out
    std::vector<std::thread> workers;
    bool quit = false;
    explicit Pool(int nw) {
      for (int t = 0; t < nw; t++)
        workers.emplace_back([this] {
          for (;;) {
            std::shared_ptr<Region> r;
            {
              std::unique_lock<std::mutex> g(mu);
              cv.wait(g, [&] {
                while (!open.empty() && open.front()->next.load() >= open.front()->n) open.pop_front();
                return quit || !open.empty();
              });
              if (open.empty()) return;
              r = open.front();  // (to the back: the next worker takes another caller's region -- the lanes share the
              open.pop_front();  // workers instead of queueing behind each other)
              open.push_back(r);
            }
            r->run();
          }
        });
    }
    ~Pool() {
      {
        std::lock_guard<std::mutex> g(mu);
        quit = true;
      }
      cv.notify_all();
      for (auto &t : workers) t.join();
    }
  };
  static Pool pool(nthreads);
  auto region = std::make_shared<Region>();
  region->body = &body;
  region->n = n;
  {
    std::lock_guard<std::mutex> g(pool.mu);
    pool.open.push_back(region);
  }
  pool.cv.notify_all();
  region->run();
  if (region->done.load() < n) {  // (workers still inside their last items: sleep, a spinning caller eats CPU quota)
    std::unique_lock<std::mutex> g(region->fin_mu);
    region->fin_cv.wait(g, [&] { return region->done.load() >= n; });
  }
  region->error.rethrow();
}

void parallel_blocks(size_t n, size_t block, const std::function<void(size_t, size_t)> &body) {
  parallel_for((int)((n + block - 1) / block), [&](int b) { body((size_t)b * block, std::min(n, ((size_t)b + 1) * block)); });
}

void run_lanes(int n, FirstError &failure, const std::function<void(int)> &body) {
  auto one = [&](int l) {
    try {
      body(l);
    } catch (...) {
      failure.set();
    }
  };
  std::vector<std::thread> threads;
  for (int l = 1; l < n; l++) threads.emplace_back(one, l);
  one(0);
  for (auto &t : threads) t.join();
}

}  // namespace sdfh
