// Context, device / pinned buffers and the planning threads shared by the pieces of the C-ABI layer; the kernels they launch
// are declared in sdf_kernels.h, the sizes they reserve come from extz2_geom.h
// (sdf_context.hip: a context's lifecycle; sdf_plan.hip: batch cutting and chunk planning; sdf_launch.hip: uploads and
// launches; sdf_api.hip and sdf_*_api.hip: entry points, by family; sdf_entry.h: the checks those share).
#pragma once
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "extz2_geom.h"
#include "sdf_kernels.h"

namespace sdf {
// (diagnostics of buffers that have no context to ask: set by every sdf_create from its configuration's debug_timing)
inline std::atomic<bool> g_debug_timing{false};

using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
inline double ms_since(Clock::time_point t0) { return ms_between(t0, Clock::now()); }

// The sections of a set-up or a call on stderr (SDF_DEBUG_TIMING).  fmt takes a section's name and its milliseconds;
// over_ms: only the sections that took longer.
struct Lap {
  bool on;
  const char *fmt;
  double over_ms = -1;
  Clock::time_point t0 = Clock::now(), last = t0;
  void operator()(const char *what) {  // since the section before
    const auto t = Clock::now();
    if (on && ms_between(last, t) > over_ms) fprintf(stderr, fmt, what, ms_between(last, t));
    last = t;
  }
  void at(const char *what) const {  // since the start
    if (on) fprintf(stderr, fmt, what, ms_since(t0));
  }
};

struct DevBuf {
  // bytes obtained by the hipMalloc calls below minus bytes given back by the hipFree calls (sdf_debug_live_device_bytes)
  static inline std::atomic<long long> live_bytes{0};
  void *p = nullptr;
  size_t cap = 0;
  // BORROWED: p / cap name memory another DevBuf holds (sdf_pool_share: a view of the owner's resident pool).  Such a buffer
  // counts no bytes, frees nothing and is never retired; whoever wants memory of its own here calls drop_borrow() first
  // (reserve() does, when it has to grow).
  bool borrowed = false;
  void borrow(void *ptr, size_t bytes) {
    release();
    p = ptr;
    cap = bytes;
    borrowed = true;
  }
  void drop_borrow() {
    if (!borrowed) return;
    p = nullptr;
    cap = 0;
    borrowed = false;
  }
  // `limit`: no headroom beyond this many bytes (the direction-flag workspace: the context's budget)
  hipError_t reserve(size_t bytes, size_t limit = ~(size_t)0) {
    if (bytes <= cap) return hipSuccess;
    drop_borrow();
    const bool dbg_t = g_debug_timing.load(std::memory_order_relaxed);
    const auto t0 = Clock::now();
    const size_t old = cap;
    // hipFree waits for the whole DEVICE -- the other lanes' batches included: 100-170 ms measured in a stage run, where
    // the allocation itself takes 0.2 ms -- so an outgrown buffer is only retired here: work of THIS call may still use it.
    // Buffers retired during EARLIER calls (new_call() has moved them to `stale`) are idle and are freed now, in the stall
    // this growth costs anyway: a context holds its buffer and at most the one it outgrew last (every outgrown
    // buffer used to stay until the context died).
    release_stale();
    if (p) {
      retired.push_back(p);
      retired_bytes += cap;
    }
    p = nullptr;
    cap = 0;
    size_t want = bytes + std::min<size_t>(bytes / 2, (size_t)8 << 30) + 4096;
    if (want > limit) want = std::max(bytes, limit);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {  // short of memory: give the retired buffers back first, then without headroom
      (void)hipGetLastError();
      for (void *q : retired) (void)hipFree(q);
      live_bytes -= (long long)retired_bytes;
      retired.clear();
      retired_bytes = 0;
      e = hipMalloc(&p, want);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        e = hipMalloc(&p, want);
      }
    }
    if (e == hipSuccess) live_bytes += (long long)(cap = want);
    if (dbg_t && want >= (64u << 20)) fprintf(stderr, "[DevBuf %zu -> %zu MiB in %.1f ms]\n", old >> 20, want >> 20, ms_since(t0));
    return e;
  }
  // without headroom (sdf_reserve: the caller's bound IS the headroom)
  hipError_t reserve_exact(size_t bytes) { return reserve(bytes, bytes); }
  // at the start of a batch call (nothing of the context's earlier calls is in flight): what earlier calls retired is idle
  // from here on -- freed at the next growth, or right away when it is more than `keep` bytes
  void new_call(size_t keep = (size_t)4 << 30) {
    stale.insert(stale.end(), retired.begin(), retired.end());
    stale_bytes += retired_bytes;
    retired.clear();
    retired_bytes = 0;
    if (stale_bytes > keep) release_stale();
  }
  void release_stale() {
    for (void *q : stale) (void)hipFree(q);
    live_bytes -= (long long)stale_bytes;
    stale.clear();
    stale_bytes = 0;
  }
  void release() {
    drop_borrow();
    if (p) (void)hipFree(p);
    for (void *q : retired) (void)hipFree(q);
    live_bytes -= (long long)(cap + retired_bytes);
    retired.clear();
    retired_bytes = 0;
    release_stale();
    p = nullptr;
    cap = 0;
  }
  size_t held_bytes() const { return (borrowed ? 0 : cap) + retired_bytes + stale_bytes; }
  std::vector<void *> retired, stale;
  size_t retired_bytes = 0, stale_bytes = 0;
};

struct HostBuf {  // pinned host memory
  void *p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    retire();  // (hipHostFree waits for the device like hipFree: freed with the context)
    // (pinning is slow -- about a millisecond per 4 MB -- and a stage run sees its batches grow: half as much again as
    // headroom, so that a context re-pins a few times, not for every batch)
    const size_t want = bytes + bytes / 2 + 4096;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  hipError_t reserve_exact(size_t bytes) {  // (sdf_reserve: no headroom on top of the caller's bound)
    if (bytes <= cap) return hipSuccess;
    retire();
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  // Large staging the HOST fills (a super-batch's characters): memory of the process's own on transparent huge pages,
  // registered with the runtime.  Measured (profiles/pin_probe.py, 182 MB): hipHostMalloc 27-30 ms + 15-22 ms to free;
  // aligned_alloc(2 MB) + MADV_HUGEPAGE + hipHostRegister 0.5 ms once the pages exist, and the pages come with the first
  // write of the threads that fill them (11 ms of zero-fill for all of it against 33-36 ms on 4 KB pages); uploads from it
  // run at the same 55 GB/s.  Falls back to hipHostMalloc where registering fails.
  hipError_t reserve_huge(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    retire();
    const size_t two_mb = (size_t)2 << 20, want = (bytes + two_mb - 1) / two_mb * two_mb;
    void *q = aligned_alloc(two_mb, want);
    if (q) {
      (void)madvise(q, want, MADV_HUGEPAGE);
      if (hipHostRegister(q, want, hipHostRegisterDefault) == hipSuccess) {
        p = q;
        cap = want;
        registered = true;
        return hipSuccess;
      }
      (void)hipGetLastError();
      free(q);
    }
    return reserve_exact(bytes);
  }
  hipError_t reserve_pinned(bool registered_huge, size_t bytes) { return registered_huge ? reserve_huge(bytes) : reserve_exact(bytes); }
  void retire() {  // the buffer in use is outgrown: kept until the context goes (each kind on its own list)
    if (p) (registered ? retired_reg : retired).push_back(p);
    p = nullptr;
    cap = 0;
    registered = false;
  }
  void release() {
    if (p) {
      if (registered) {
        (void)hipHostUnregister(p);
        free(p);
      } else {
        (void)hipHostFree(p);
      }
    }
    for (void *q : retired) (void)hipHostFree(q);
    for (void *q : retired_reg) {
      (void)hipHostUnregister(q);
      free(q);
    }
    retired.clear();
    retired_reg.clear();
    p = nullptr;
    cap = 0;
    registered = false;
  }
  std::vector<void *> retired, retired_reg;
  bool registered = false;
};

struct BatchCut;

// A few parked host threads for the planning of a batch (a thread costs ~0.1 ms to start and join, a planning pass over
// a hundred thousand tasks less than a millisecond: the threads are started once per context).
class WorkerPool {
 public:
  explicit WorkerPool(int n, int spin_us = 0) {
    spin_us_ = spin_us > 0 ? spin_us : 0;
    for (int t = 0; t < n; ++t) threads_.emplace_back([this] { loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    for (auto &t : threads_) t.join();
  }
  int size() const { return (int)threads_.size(); }
  void submit(std::function<void()> job) {
    {
      std::lock_guard<std::mutex> g(mu_);
      jobs_.push_back(std::move(job));
      ++pending_;
      njobs_.fetch_add(1, std::memory_order_release);
    }
    cv_.notify_one();
  }
  void wait_idle() {  // every submitted job has finished
    std::unique_lock<std::mutex> g(mu_);
    idle_.wait(g, [&] { return pending_ == 0; });
  }

 private:
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        // A parked thread takes 0.1 - 3 ms to wake up on a box with a CPU quota -- as long as the whole scan of a million
        // tasks it is woken for.  SDF_POOL_SPIN_US lets a thread keep looking for the next job for a while before it
        // parks.  Off by default: measured on the 40,000-pair stage run (three lanes, 16-CPU quota) 300 us of looking cost
        // more in throttled periods than it saved -- 0.42-0.95 s per run against 0.32-0.46 s.
        const auto t0 = std::chrono::steady_clock::now();
        bool got = false;
        while (!got && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us_)) {
          if (njobs_.load(std::memory_order_acquire) > 0) {
            std::lock_guard<std::mutex> g(mu_);
            if (!jobs_.empty()) {
              job = std::move(jobs_.front());
              jobs_.pop_front();
              njobs_.fetch_sub(1, std::memory_order_release);
              got = true;
            }
          } else {
            __builtin_ia32_pause();
          }
        }
        if (!got) {
          std::unique_lock<std::mutex> g(mu_);
          cv_.wait(g, [&] { return quit_ || !jobs_.empty(); });
          if (jobs_.empty()) return;
          job = std::move(jobs_.front());
          jobs_.pop_front();
          njobs_.fetch_sub(1, std::memory_order_release);
        }
      }
      job();
      {
        std::lock_guard<std::mutex> g(mu_);
        if (--pending_ == 0) idle_.notify_all();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::deque<std::function<void()>> jobs_;
  std::mutex mu_;
  std::condition_variable cv_, idle_;
  int pending_ = 0;
  bool quit_ = false;
  std::atomic<int> njobs_{0};
  int spin_us_ = 0;  // sdf_config.pool_spin_us (set_spin_us)
};
}
using sdf::DevBuf;
using sdf::HostBuf;

// Every device buffer of a context, one X(name, group) each: the members of sdf_ctx, and what sdf_destroy releases and
// sdf_device_bytes sums.  `group`: the calls at whose start the buffer is renewed (DevBuf::new_call: what it outgrew in
// earlier calls is idle and may be freed) -- BatchCall: batch_part; Pairs: batch_pairs, sdf_pool_range_classes; Pool: sdf_pool_append_fasta
// (sdf_pool_upload: an_pool alone); None: never, what such a buffer outgrows stays until the context goes.
enum class BufGroup { Any, None, BatchCall, Pairs, Pool };
#define SDF_DEVICE_BUFFERS(X)                                                                                        \
  X(dir_ws, BatchCall)   /* direction flags of the chunks in flight: the context's workspace */                       \
  X(stage_ws, BatchCall) /* CIGAR staging slots */                                                                    \
  X(plan_buf, BatchCall)                                                                                              \
  X(order_buf, BatchCall)                                                                                             \
  X(misc_buf, None)                                                                                                   \
  X(gstate_buf, BatchCall)                                                                                            \
  X(an_pool, Pool) /* the resident characters (pool_bytes of them) */                                                 \
  X(an_pairs, None) X(an_keys, None) X(an_keys2, None) X(an_q, None) X(an_off, None) X(an_flag, None) /* anchors calls */ \
  X(an_pos, None) X(an_cand, None) X(an_out, None) X(an_tmp, None) X(an_outoff, None)                                 \
  X(ch_an, None) X(ch_off, None) X(ch_wsoff, None) X(ch_work, None) /* sdf_chain_batch */                             \
  X(ch_path, None) X(ch_bounds, None) X(ch_nb, None) X(ch_which, None)                                                \
  X(st_tasks, None) X(st_pool, None) X(st_cig, None) X(st_out, None) /* sdf_stats_columns_batch */                    \
  X(claim_buf, None)   /* stripe launches: eight entry counters each (stripe_claim), zeroed per call */               \
  X(st_items, None)    /* sdf_stats_columns_device: segments of long alignments + their counter */                    \
  X(sc_counts, None) /* sdf_stats_cuts_pairs_device: per alignment the count word and {matches, span} */              \
  X(sc_tasks, None) X(sc_cig, None) X(sc_first, None) X(sc_out, None) /* sdf_stats_cuts_pairs: the host form's copies */ \
  X(mz_plan, None) X(mz_counts, None) /* sdf_pool_minimizers_device: blocks per range / records per block, and their scans */ \
  X(mz_ranges, None) X(mz_first, None) X(mz_out, None) /* sdf_pool_minimizers: the host form's copies */               \
  X(mz_keys, None) X(mz_vals, None) X(mz_groups, None) X(mz_tmp, None) /* sdf_pool_minimizer_index: sort keys (in, out), */ \
  X(mz_sorted, None) X(mz_res, None) /* ... places (in, out), heads / ranks / starts, sort scratch, sorted records, results */ \
  X(sw_keys, None) X(sw_vals, None) X(sw_tmp, None) /* sdf_search_windows_device: sort keys and places (in, out), sort scratch, */ \
  X(sw_look, None) X(sw_counts, None) /* ... a SearchLook per query minimizer, intervals per window */                  \
  X(sw_wide, None) X(sw_nwide, None) /* sdf_search_windows_wide_device: the listed window indices, the number of eligible windows */ \
  X(sw_q, None) X(sw_r, None) X(sw_limit, None) X(sw_first, None) X(sw_win, None) X(sw_out, None) /* sdf_search_windows: the host form's copies */ \
  X(fo_counts, None) X(fo_start, None) X(fo_ent, None) X(fo_need, None) X(fo_tmp, None) /* the bin index of the found records: counts / cursors, bin starts, entries, the need, hipCUB scratch */ \
  X(fo_found, None) X(fo_vis, None) X(fo_q, None) X(fo_first, None) X(fo_rolls, None) X(fo_out, None) /* sdf_search_windows_found, sdf_search_overlap: the host forms' copies */ \
  X(sr_q, None) X(sr_win, None) X(sr_first, None) X(sr_iv, None) X(sr_r, None) X(sr_limit, None) X(sr_out, None) /* sdf_search_roll: the host form's copies */ \
  X(sf_tasks, None) X(sf_out, None) /* sdf_search_filter: the host form's copies */ \
  X(se_rolls, None) X(se_filter, None) X(se_out, None) /* sdf_search_extend: the host form's copies (the rest: sdf_search_roll's) */ \
  X(sl_ws, None) X(sl_tmp, None) /* sdf_search_extend_long_device: flags, list, a batch's keys / payloads / heads / slots; hipCUB scratch */ \
  X(ac_win, None) X(ac_kept, None) X(ac_off, None) X(ac_go, None) /* sdf_search_accept_device: an AcceptWin and an AcceptOff per round window, the kept entries, the windows the append may write */ \
  X(ac_in, None) X(ac_found, None) X(ac_out, None) X(ac_status, None) /* sdf_search_accept: the host form's copies (the round's arrays in one piece) */ \
  X(dr_q, None) X(dr_r, None) X(dr_rs, None) X(dr_limit, None) X(dr_found, None) /* sdf_search_pair: minimizers of both ranges, the reference's index, the limit table, the found list */ \
  X(dr_first, None) X(dr_win, None) X(dr_vis, None) X(dr_act, None) X(dr_iv, None) X(dr_rolls, None) X(dr_tasks, None) X(dr_verd, None) /* ... a round: per window, per interval */ \
  X(dr_frec, None) X(dr_hits, None) X(dr_htasks, None) X(dr_hrec, None) X(dr_out, None) X(dr_status, None) /* ... the round's hits and status (with the two needs behind it) */ \
  X(h_pool, BatchCall) X(h_out, BatchCall) X(h_cig, BatchCall) /* device buffers of the host-buffer entry point */    \
  X(h_brief, BatchCall) /* ... 16-byte result records (sdf_extz2_batch_brief) */                                      \
  X(pk_recs, Pairs)     /* one PackRec per task of an sdf_extz2_batch_pairs call (seq_pack.hip) */                    \
  X(cl_ranges, Pairs) X(cl_out, Pairs) /* sdf_pool_range_classes: a ClassRange and a record of four counts per range */ \
  X(pf_recs, None) X(pf_out, None) /* sdf_pool_fetch_ranges: a piece's FetchRec records and its output bytes (fetch_stage_bytes) */ \
  X(cv_regions, None) X(cv_iv, None) X(cv_upper, None) X(cv_out, None) /* sdf_pool_coverage: a CoverRegion per region, a CoverIv and a count per interval, seven counters per region */ \
  X(cv_bits, None) /* ... the bitmaps: a bit per base of every region, set 0 then set 1 (pool_cover.hip), zeroed per call */ \
  X(bk_ws, None) X(bk_tmp, None) /* sdf_bucket_merge_device: records, sort keys and places, scan items, runs, slots (sdf_bucket_api.hip: bucket_launch); hipCUB scratch */ \
  X(bk_in, None) X(bk_chr, None) X(bk_pairs, None) X(bk_out, None) /* sdf_bucket_merge: the host form's copies (the two counts in front of the records) */ \
  X(sd_in, None) X(sd_out, None) /* sdf_seed_records: the host form's copies (hits, first[], the job table in one piece; the records) */ \
  X(rc_ws, None) X(rc_tmp, None) /* sdf_pair_recall_device: the longest end, the entries as made and as sorted (sdf_recall_api.hip: recall_launch); hipCUB scratch */ \
  X(rc_gold, None) X(rc_found, None) X(rc_out, None) /* sdf_pair_recall: the host form's copies (the two status words in front of the results) */ \
  X(lo_ws, None) X(lo_tmp, None) /* sdf_line_order_device: the listed runs' count, sort keys and places twice, head bytes, the list (sdf_report_api.hip: lines_launch); hipCUB scratch */ \
  X(lo_pool, None) X(lo_lines, None) X(lo_out, None) /* sdf_line_order: the host form's copies (the three counts in front of order and flags) */ \
  X(sd_tab, None) X(sd_merged, None) /* sdf_seeds_bucket_merge: the two tables of the merge in one piece; the two counts in front of the merged records */ \
  X(fa_raw, Pool) /* a piece of a FASTA record's lines on their way into an_pool (sdf_pool_append_fasta) */           \
  /* lane kernel (extz2_lane.hip): records as uploaded, sort keys / values (in, out), sizes and their scans, hipCUB scratch */ \
  X(ln_recs, BatchCall) X(ln_keys, BatchCall) X(ln_vals, BatchCall) X(ln_sizes, BatchCall) X(ln_tmp, BatchCall)       \
  X(ln_bins, None) /* ... second form of the lane planning: per-key counts, ranks, prefixes (lane_hist_kernel and on) */ \
  /* outputs of rerun_ctx, and the (record, staging slot) map of the merge */                                         \
  X(rr_out, None) X(rr_cig, None) X(rr_map, None)
// ... and every pinned host buffer
#define SDF_HOST_BUFFERS(X)                                                                                          \
  X(host_plan) /* pinned staging of the plan (two) */                                                                 \
  X(host_order)                                                                                                       \
  X(host_pool) /* pinned staging of the host-buffer entry point: packed sequences; results + CIGARs */                \
  X(host_out)                                                                                                         \
  X(host_lane)  /* the lane kernel's records */                                                                       \
  X(host_chars) /* pinned staging of a super-batch's FASTA characters (sdf_pool_host) */                              \
  X(host_cls) /* sdf_pool_range_classes: the ranges' records on their way up, the counts on their way back */          \
  X(host_fetch) /* sdf_pool_fetch_ranges: a piece's output on its way back, its records behind it on their way up */  \
  X(host_an) /* pinned staging of the anchors call's output (sdf_reserve with SDF_RESERVE_ANCHORS; a pageable copy runs at ~3 GB/s) */

// A resident search index (include/sedef_hip.h: sdf_search_index_build): one range's minimizers in ascending loc and its sorted
// index, on the host (the driver's schedule and host step) and in HBM, in buffers of its own.  Its context lists it and frees
// it with itself; pool_epoch: the context's when the handle was built -- a pool replaced since then makes the handle stale.
struct sdf_search_index {
  sdf_ctx *ctx = nullptr;
  uint64_t pool_epoch = 0;
  sdf_minim_range range{0, 0, 0};
  int k = 0, w = 0, separate_lowercase = 0;
  uint32_t threshold = 0x80000000u, n_groups = 0;
  std::vector<sdf_minimizer> loc, sorted;
  DevBuf d_loc, d_sorted;
};

// The lanes of sdf_search_pairs_indexed (include/sedef_hip.h: sdf_search_lanes_open; sdf_lanes_api.hip): child contexts of
// `owner`, each a view of the owner's pool with a stream and per-call buffers of its own.  The owner lists the object and
// closes it with itself.
struct sdf_search_lanes {
  sdf_ctx *owner = nullptr;
  std::vector<sdf_ctx *> lane;
};

struct sdf_ctx {
  sdf_config cfg;  // the context's settings, fixed when it is made (sdf_config.hip): every setting is read from here
  int device = 0;
  hipStream_t stream = nullptr;
  size_t ws_budget = 0;
  hipStream_t dp_stream[2] = {nullptr, nullptr}, tb_stream = nullptr;  // chunk pipeline
  hipStream_t wide_stream[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // chunks of several mixed-pair launches (sdf_launch.hip)
  size_t aux_limit = 4;  // extra pipeline streams this context may create (sdf_reserve with SDF_RESERVE_FEW_STREAMS: 0)
  hipStream_t aux_stream[4] = {nullptr, nullptr, nullptr, nullptr};    // more room for launches that end in a tail
  hipStream_t lane_stream = nullptr;
#define X(name, group) DevBuf name;
  SDF_DEVICE_BUFFERS(X)
#undef X
#define X(name) HostBuf name;
  SDF_HOST_BUFFERS(X)
#undef X
  std::vector<sdf_task> host_tasks;  // the task array of the host-buffer entry point with word offsets
  size_t pool_bytes = 0;   // characters resident in an_pool (sdf_pool_upload / sdf_anchors_batch): what sdf_extz2_batch_pairs may name
  uint64_t pool_epoch = 0; // grows whenever the pool is REPLACED (an upload, a reset, a view taken or dropped), not when it is appended to
  std::vector<sdf_search_index *> indexes;  // the live handles of sdf_search_index_build (sdf_driver_api.hip); sdf_destroy frees them
  long long index_builds = 0;               // sdf_search_index_build calls that returned a handle
  std::vector<sdf_search_lanes *> lanes;    // the open lanes of sdf_search_lanes_open (sdf_lanes_api.hip); sdf_destroy closes them
  long long lane_tasks = 0;   // tasks of the last batch call the lane kernel took
  // sdf_last_chain_classes: pairs of the last sdf_chain_batch per launch class -- [0..5] the LDS classes of chain_wave_kernel,
  // [6] chain_kernel --, [7] the LDS cap of class 5 in bytes (fixed in sdf_create: what the kernel was granted there)
  int64_t chain_classes[8] = {0, 0, 0, 0, 0, 0, 0, 64 * 1024};
  // sdf_last_traceback_classes: launches of traceback_kernel<layout, G> in the last batch call, [2 * layout + (G == 16)];
  // counted on the host where they are launched (sdf_launch.hip), zeroed when a batch call starts
  int64_t tb_classes[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  sdf::WorkerPool *pool = nullptr;  // planning threads, started with the first batch large enough to use them
  sdf::BatchCut *cut = nullptr;  // chunk list and planning scratch of the last batch call (sdf_plan.hip)
  std::vector<hipEvent_t> events;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // 0 DP, 1 traceback, 2 compaction, 3 stream total, 4 host planning before the
                                           // first launch, 5 host total, 6 sum of the chunks' DP intervals
  int launches = 0;
  long long paired = 0;  // tasks of the last batch that ran two per wavefront (extz2_pair.hip)
  std::string err;
  int max_dyn_lds = 64 * 1024;  // dynamic LDS the general kernels may ask for (raised in sdf_create where the device allows)
  bool pipeline_ok = true;      // cfg.pipeline, and the pipeline's streams could be created (else one chunk on one stream)
  sdf_ctx *part_ctx = nullptr;    // second context of this device: the first part of a very large batch (sdf_api.hip)
  hipEvent_t part_ev = nullptr;
  bool is_part = false, pool_shared = false;
  // sdf_pool_share (sdf_context.hip): a VIEW borrows its owner's an_pool and names the owner here; the owner lists its views.
  // Both sides are touched under one process-wide lock, by sdf_pool_share, by whatever gives a view a pool of its own again
  // (pool_writable) and by sdf_destroy.
  sdf_ctx *view_of = nullptr;
  std::vector<sdf_ctx *> views;
  sdf_ctx *rerun_ctx = nullptr;   // context without stripe kernels for the tasks they gave up (created when first needed)
  long long reran = 0;            // tasks of the last batch call that were re-run after a stripe gave up
};

// f(DevBuf &) for every device buffer of a context, or for those of one group; f(HostBuf &) for every pinned one
template <class Ctx, class F>
inline void for_each_device_buffer(Ctx *ctx, F &&f, BufGroup only = BufGroup::Any) {
#define X(name, group) if (only == BufGroup::Any || only == BufGroup::group) f(ctx->name);
  SDF_DEVICE_BUFFERS(X)
#undef X
}
template <class F>
inline void for_each_host_buffer(sdf_ctx *ctx, F &&f) {
#define X(name) f(ctx->name);
  SDF_HOST_BUFFERS(X)
#undef X
}
// f(hipStream_t &) for every stream of a context, created or not: the one place that lists them
template <class F>
inline void for_each_stream(sdf_ctx *ctx, F &&f) {
  f(ctx->stream);
  for (hipStream_t &q : ctx->dp_stream) f(q);
  f(ctx->tb_stream);
  for (hipStream_t &q : ctx->aux_stream) f(q);
  for (hipStream_t &q : ctx->wide_stream) f(q);
  f(ctx->lane_stream);
}

// a context another context owns (the first part of a split batch, the re-run of abandoned stripe tasks): not another
// user of the process's CPUs (sdf_context.hip, like the two below)
void mark_internal_context(sdf_ctx *c);
// sdf_create_cfg with a say on the chunk pipeline's three streams: a context that never runs a DP batch (a search lane) does
// without them
sdf_ctx *create_context(int device, size_t workspace_bytes, const sdf_config *cfg_in, bool pipeline_streams);
// the lanes of a list entry destroyed, the entry gone from its owner's list (sdf_lanes_api.hip)
void close_lanes(sdf_ctx *owner, sdf_search_lanes *lanes);
// In front of everything that replaces or grows a context's resident pool.  SDF_ERR_INVALID ("pool is shared"): other
// contexts view this one's pool, or -- keep_view -- this context holds a view and the caller wants to add to it.  Otherwise
// SDF_OK, and a context that held a view holds none any more: an empty pool of its own.
int pool_writable(sdf_ctx *ctx, bool keep_view = false);
extern std::atomic<int> g_live_contexts;  // contexts of this process that callers made
int usable_cpus();                        // CPUs this process may really use: the affinity mask capped by the cgroup's CPU quota

#define SDF_HIP(call)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
      return SDF_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)
