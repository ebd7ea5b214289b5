// The job queue of sdf_search_pairs_indexed (sedef_amd/csrc/sdf_job_queue.h) on its own, with a stub job and no device: built with
// -fsanitize=thread and run by tests/test_search_lanes_cpu.py.  Exit status 0 and "job queue ok" when every statement holds; a
// data race makes the sanitizer's runtime end the program with a status of its own.
#include <cstdio>
#include <cstdlib>
#include <new>

#include "sdf_job_queue.h"

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s fails\n", __LINE__, #cond);    \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main() {
  using namespace sdf;
  // the largest first, equal sizes by index
  CHECK((largest_first({5, 9, 5, 1, 9}) == std::vector<size_t>{1, 4, 0, 2, 3}));
  CHECK(largest_first({}).empty());
  for (size_t n_lanes : {1, 2, 4, 16}) {
    // every job once, on a lane below n_lanes, never more than n_lanes at a time; a lane's own state needs no lock
    const size_t n = 500;
    std::vector<uint64_t> size(n);
    for (size_t j = 0; j < n; j++) size[j] = (j * 7919) % 101;
    std::vector<int> runs(n, 0), lane_of(n, -1);
    std::vector<long long> lane_sum(n_lanes, 0);  // (what a lane's buffers are to a job: touched by that lane's thread alone)
    std::atomic<int> in_flight{0}, most{0};
    const std::vector<int> code = run_job_queue(n_lanes, largest_first(size), [&](size_t lane, size_t job) {
      const int now = in_flight.fetch_add(1) + 1;
      int seen = most.load();
      while (now > seen && !most.compare_exchange_weak(seen, now)) {}
      runs[job] += 1, lane_of[job] = (int)lane;
      lane_sum[lane] += (long long)size[job];
      in_flight.fetch_sub(1);
      return 0;
    });
    long long sum = 0, want = 0;
    for (size_t j = 0; j < n; j++) {
      CHECK(code[j] == 0 && runs[j] == 1 && lane_of[j] >= 0 && (size_t)lane_of[j] < n_lanes);
      want += (long long)size[j];
    }
    for (long long s : lane_sum) sum += s;
    CHECK(sum == want && most.load() >= 1 && (size_t)most.load() <= n_lanes);
  }
  {  // fewer jobs than lanes: the spare lanes stay idle; no job at all
    std::vector<int> lane_of(2, -1);
    const std::vector<int> code = run_job_queue(16, {1, 0}, [&](size_t lane, size_t job) { return lane_of[job] = (int)lane, 0; });
    CHECK(code == (std::vector<int>{0, 0}) && lane_of[0] >= 0 && lane_of[0] < 2 && lane_of[1] >= 0 && lane_of[1] < 2);
    CHECK(run_job_queue(4, {}, [&](size_t, size_t) { return abort(), 0; }).empty());
  }
  {  // a job that fails: on one lane nothing behind it in the order is started
    std::vector<int> runs(6, 0);
    const std::vector<int> code = run_job_queue(1, {3, 1, 4, 0, 5, 2}, [&](size_t, size_t job) { return runs[job] += 1, job == 4 ? -2 : 0; });
    CHECK((code == std::vector<int>{kJobNotStarted, 0, kJobNotStarted, 0, -2, kJobNotStarted}));
    CHECK((runs == std::vector<int>{0, 1, 0, 1, 1, 0}));
  }
  for (size_t n_lanes : {2, 4, 16}) {  // ... on several lanes: the jobs that were started have their codes, the rest was not run
    const size_t n = 400;
    std::vector<size_t> order(n);
    for (size_t j = 0; j < n; j++) order[j] = j;
    std::vector<int> runs(n, 0);
    const std::vector<int> code = run_job_queue(n_lanes, order, [&](size_t, size_t job) { return runs[job] += 1, job == 37 ? -6 : 0; });
    for (size_t j = 0; j < n; j++) CHECK(code[j] == (j == 37 ? -6 : runs[j] ? 0 : kJobNotStarted) && runs[j] <= 1);
    // (the jobs in front of the failing one were taken off the queue before it was, hence before it failed)
    for (size_t j = 0; j <= 37; j++) CHECK(runs[j] == 1);
  }
  {  // a job that throws: caught on its lane's thread, a failure like any other
    std::vector<int> runs(5, 0);
    const std::vector<int> code = run_job_queue(1, {0, 1, 2, 3, 4}, [&](size_t, size_t job) {
      runs[job] += 1;
      if (job == 2) throw std::bad_alloc();
      return 0;
    });
    CHECK((code == std::vector<int>{0, 0, kJobThrew, kJobNotStarted, kJobNotStarted}) && (runs == std::vector<int>{1, 1, 1, 0, 0}));
    std::atomic<int> ran{0};
    const std::vector<int> many = run_job_queue(4, {0, 1, 2, 3, 4, 5, 6, 7}, [&](size_t, size_t job) -> int {
      ran.fetch_add(1);
      if (job == 0) throw 7;
      return 0;
    });
    CHECK(many[0] == kJobThrew && ran.load() >= 1);
    for (size_t j = 1; j < many.size(); j++) CHECK(many[j] == 0 || many[j] == kJobNotStarted);
  }
  printf("job queue ok\n");
  return 0;
}
