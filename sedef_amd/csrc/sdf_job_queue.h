// The job queue of sdf_search_pairs_indexed (sdf_lanes_api.hip): independent jobs taken off one shared queue by one host thread
// per lane.  Plain C++ without a device, so that a program of its own can run it under a thread sanitizer with a stub job
// (tests/job_queue_main.cc).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <thread>
#include <vector>

namespace sdf {
constexpr int kJobNotStarted = 1;  // (no SDF_* code is positive)
constexpr int kJobThrew = 2;       // work() left by an exception: caught on the lane's thread, the job counts as failed

// the order in which the queue hands the jobs out: the largest first, equal sizes by index -- the tail of a call is short
inline std::vector<size_t> largest_first(const std::vector<uint64_t> &size) {
  std::vector<size_t> order(size.size());
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return size[a] > size[b]; });
  return order;
}

// work(lane, job) -> 0 or a code, for every job of `order` until one fails: min(n_lanes, jobs) threads, thread t is lane t for its
// whole life, all joined before this returns.  After a job has failed no further job is started; those that run finish.
// Returns a code per job (indexed by job, not by place in the order): work's, kJobThrew for a job whose work threw, or
// kJobNotStarted.  No exception leaves a lane's thread.  A thread that cannot be started is done without: the threads that
// exist take its jobs, and with none at all the caller's thread is lane 0.
template <class Work>
inline std::vector<int> run_job_queue(size_t n_lanes, const std::vector<size_t> &order, Work &&work) {
  const size_t n = order.size();
  std::vector<int> code(n, kJobNotStarted);
  std::atomic<size_t> next{0};
  std::atomic<bool> stop{false};
  const auto lane_loop = [&](size_t lane) {
    while (!stop.load(std::memory_order_acquire)) {
      const size_t at = next.fetch_add(1, std::memory_order_relaxed);
      if (at >= n) break;
      const size_t job = order[at];
      int rc = kJobThrew;
      try {
        rc = work(lane, job);
      } catch (...) {
      }
      code[job] = rc;  // (each job is taken once: no two threads write one entry)
      if (rc != 0) stop.store(true, std::memory_order_release);
    }
  };
  std::vector<std::thread> threads;
  const size_t n_threads = std::min(n_lanes, n);
  try {
    threads.reserve(n_threads);
    for (size_t t = 0; t < n_threads; t++) threads.emplace_back(lane_loop, t);
  } catch (...) {  // (no room or no thread to be had: on with those that started)
  }
  if (threads.empty() && n) lane_loop(0);
  for (std::thread &t : threads) t.join();
  return code;
}
}  // namespace sdf
