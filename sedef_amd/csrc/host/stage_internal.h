// What the files of the `align generate` stage share and sedef_host.h does not export: the host threads (host_threads.cc), the
// clocks and counters of a run (pair_job.cc, stage_driver.cc), the test hook of a DP request's chunks (dp_provider.cc).
#pragma once
#include <atomic>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <thread>

#include "sedef_host.h"

namespace sdfh {

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }  // seconds

// body(0 .. n - 1) on the host threads of the process (SDF_HOST_THREADS; one pool serves every caller): returns when all are
// done, the first failure rethrown as a std::string.  parallel_blocks: body(lo, hi) for every block [lo, hi) of [0, n).
void parallel_for(int n, const std::function<void(int)> &body);
void parallel_blocks(size_t n, size_t block, const std::function<void(size_t, size_t)> &body);

// The first failure of the threads that work for one caller: recorded in their catch blocks -- whatever was thrown --, rethrown
// on the caller's thread, once they have all returned, as the std::string message the stage's callers handle.
class FirstError {
 public:
  void set();  // (inside a catch block)
  bool failed() const { return failed_; }
  void rethrow() const {
    if (failed_) throw msg_;
  }

 private:
  std::mutex mu_;
  std::atomic<bool> failed_{false};
  std::string msg_;
};
// body(0) on the calling thread, body(1 .. n - 1) on threads of their own, until all have returned; the first failure of any
// of them is left in `failure` (which tells the others that one has failed) for the caller to rethrow.
void run_lanes(int n, FirstError &failure, const std::function<void(int)> &body);

struct StageTotals {  // stage_totals(): of the process since stage_totals_reset()
  std::atomic<long long> records{0}, chars{0}, batches{0}, batches_resident{0};
};
extern StageTotals g_totals;
extern std::atomic<long long> g_us_chain, g_us_rest;  // host CPU time of the pair jobs (summed over threads), microseconds

// TEST HOOK (sdfh_dp_chunks): the chunks of one request as the providers cut them, four values each (room for `cap` chunks)
size_t dp_chunks(int qlen, int tlen, size_t step, bool t_rc, int64_t t_off, long long *out, size_t cap);

}  // namespace sdfh
