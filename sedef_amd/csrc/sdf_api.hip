// The C ABI (include/sedef_hip.h): packing helpers and the DP batch entry points (the context itself: sdf_context.hip; the
// resident pool, seeding, stats and minimizers: sdf_pool_api.hip, sdf_seed_api.hip, sdf_stats_api.hip, sdf_minim_api.hip).
// Replaces the call site of ksw_extz2_sse in align_helper (reference: src/align.cc:39-68) with a
// batched device path.  No CPU fallback exists here: every DP cell is computed by a gfx950 kernel.
// Planning lives in sdf_plan.hip, uploads and launches in sdf_launch.hip (same translation unit, see sdf_unity.hip).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "sdf_batch.h"
#include "sdf_entry.h"

using namespace sdf;

extern "C" size_t sdf_packed_words(int32_t len) {
  if (len <= 0) return 0;
  return (size_t)(len + 15) / 16 + (size_t)(len + 31) / 32;
}

extern "C" void sdf_pack_codes(const uint8_t *codes, int32_t len, uint32_t *out) {
  const size_t nw = sdf_packed_words(len);
  std::memset(out, 0, nw * sizeof(uint32_t));
  uint32_t *cw = out, *nm = out + (len + 15) / 16;
  int32_t k = 0;
  // eight bases at a time: a code >= 4 is N (mask bit set, code bits 0); codes are 0..4 in the callers, any
  // byte >= 4 is treated as N like in the byte loop below
  for (; k + 8 <= len; k += 8) {
    uint64_t x;
    std::memcpy(&x, codes + k, 8);
    // bytes >= 4 have one of bits 2..7 set: fold them onto bit 0 of each byte
    uint64_t hi = x & 0xFCFCFCFCFCFCFCFCull;
    hi |= hi >> 4;
    hi |= hi >> 2;
    hi |= hi >> 1;
    const uint64_t nb = hi & 0x0101010101010101ull;
    const uint32_t nbits = (uint32_t)((nb * 0x0102040810204080ull) >> 56);
    uint64_t y = x & 0x0303030303030303ull & ~(nb * 0xFFull);
    y = (y | (y >> 6)) & 0x000F000F000F000Full;
    y = (y | (y >> 12)) & 0x000000FF000000FFull;
    y = (y | (y >> 24)) & 0xFFFFull;
    cw[k >> 4] |= (uint32_t)y << ((k & 15) * 2);
    nm[k >> 5] |= nbits << (k & 31);
  }
  for (; k < len; ++k) {
    const uint8_t c = codes[k];
    if (c >= 4) nm[k >> 5] |= 1u << (k & 31);
    else cw[k >> 4] |= (uint32_t)c << ((k & 15) * 2);
  }
}

extern "C" size_t sdf_pack_tasks(const uint8_t *codes, const int64_t *q_off, const int32_t *qlen, const int64_t *t_off,
                                 const int32_t *tlen, size_t n, uint32_t *out, int64_t *q_word, int64_t *t_word) {
  size_t words = 0;
  for (size_t k = 0; k < n; ++k) {
    q_word[k] = (int64_t)words;
    words += sdf_packed_words(qlen[k]);
    t_word[k] = (int64_t)words;
    words += sdf_packed_words(tlen[k]);
  }
  if (out)
    for (size_t k = 0; k < n; ++k) {
      if (qlen[k] > 0) sdf_pack_codes(codes + q_off[k], qlen[k], out + q_word[k]);
      if (tlen[k] > 0) sdf_pack_codes(codes + t_off[k], tlen[k], out + t_word[k]);
    }
  return words;
}

extern "C" int64_t sdf_band_cells(int32_t qlen, int32_t tlen, int32_t w) {
  if (qlen <= 0 || tlen <= 0) return 0;
  if (w < 0) w = tlen > qlen ? tlen : qlen;
  int64_t cells = 0;
  for (int r = 0; r < qlen + tlen - 1; ++r) {
    Band b;
    if (!band_of(r, qlen, tlen, w, b)) break;
    cells += b.hi0 - b.lo0 + 1;
  }
  return cells;
}

namespace {

int make_scorek(sdf_ctx *ctx, const sdf_scoring *sc, ScoreK &k) {
  if (!sc || sc->m != 5) {
    ctx->err = "scoring: the GPU path implements the 5-letter alphabet (ACGT + wildcard) only";
    return SDF_ERR_UNSUPPORTED;
  }
  const int q = sc->gapo, e = sc->gape;
  k.q = q;
  k.e = e;
  k.qe = q + e;
  k.q_b = (uint8_t)q;
  k.qe2_b = (uint8_t)((q + e) * 2);
  k.cap_b = (uint8_t)(int8_t)(sc->mat[0] + (q + e) * 2);
  k.sc_match = (uint8_t)sc->mat[0];
  k.sc_mis = (uint8_t)sc->mat[1];
  k.wild = (uint8_t)(sc->m - 1);
  memcpy(k.mat, sc->mat, 25);
  return SDF_OK;
}

// The planning environment of a batch call -- batch_part's and sdf_debug_plan's, which plans exactly like it: the
// settings, and what the scoring (validated by make_scorek) and the request allow.  The lane kernel needs the records its
// scan fills as well (env.lane_recs: pinned memory of a context), which batch_part adds.
static PlanEnv plan_env(const sdf_config &cfg, const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want,
                        int max_dyn_lds) {
  PlanEnv env;
  env.cfg = &cfg;
  env.tasks = tasks;
  env.n = n;
  env.want = want;
  int min_sc = sc->mat[1];
  for (int t = 1; t < sc->m * sc->m; ++t) min_sc = std::min<int>(min_sc, sc->mat[t]);
  env.degenerate = -min_sc > 2 * (sc->gapo + sc->gape);  // reference returns before any work (:81)
  env.gapo = sc->gapo;
  env.max_dyn_lds = max_dyn_lds;
  // The register-resident window kernels take three differences of the recurrence with 32-bit subtracts (extz2_wave.hip:
  // SDF_CORE), which needs every fresh score byte z0 = score + 2 (q + e) in q .. 127: SEDEF's scoring and every sane one.
  // Anything else -- bytes that wrap, a mismatch below -(q + 2 e) -- runs on the general kernel, which emulates the
  // reference's bytes one by one.
  const int qe2 = 2 * (sc->gapo + sc->gape), zm = sc->mat[0] + qe2, zx = sc->mat[1] + qe2;
  const bool core32_ok = sc->gapo >= 0 && sc->gape >= 0 && zm <= 127 && zx <= 127 && zm >= sc->gapo && zx >= sc->gapo;
  env.force_general = cfg.force_general != 0 || !core32_ok;
  // the lane and strip kernels: a tame scoring (every byte of the reference's state stays in 0..127: no wrap-around, no
  // signed / unsigned or sign-extension artefacts); the lane kernel: nothing but CIGAR / score / mte wanted, the strip
  // kernels: zx - q >= 0 (they take z - q with a 32-bit subtract on packed halves, extz2_strip.hip)
  const bool tame = !env.degenerate && sc->gapo >= 0 && sc->gape >= 0 && zm >= 0 && zm <= 127 && zx >= 0 && zx <= 127;
  env.lane_ok = cfg.no_lane == 0 && cfg.force_general == 0 && tame && !(want & SDF_WANT_EXT) && n >= (size_t)cfg.lane_min;
  env.strip_ok = cfg.no_strip == 0 && cfg.force_general == 0 && tame && zx - sc->gapo >= 0 && sc->mat[0] >= 0;
  return env;
}

// Plans the chunks of a cut, in launch order, on `nthreads` worker threads; wait(ci) blocks until chunk ci is planned.
// With nthreads == 0 wait(ci) plans the chunk itself (small batches: nothing to overlap with).
class ChunkPlanner {
 public:
  // nworkers jobs on `pool` (may be null when nworkers == 0)
  // (`first`: the chunks before it have been planned and launched already -- the early start of the heavy chunks)
  ChunkPlanner(const PlanEnv &env, BatchCut &cut, PlanTask *plan, int32_t *order, WorkerPool *pool, int nworkers, size_t first = 0)
      : env_(env), cut_(cut), plan_(plan), order_(order), pool_(nworkers > 0 ? pool : nullptr),
        ready_(cut.chunks.size(), 0), first_(first) {
    if (!pool_) return;
    next_.store(first + 1);  // chunk `first` is planned by the caller of wait(first): no hand-over in front of the GPU's start
    for (int t = 0; t < nworkers; ++t) pool_->submit([this] { work(); });
  }
  ~ChunkPlanner() {
    stop_.store(true);
    if (pool_) pool_->wait_idle();
  }
  void wait(size_t ci) {
    if (!pool_ || ci == first_) {
      plan_chunk(env_, cut_, cut_.chunks[ci], plan_, order_, own_);
      return;
    }
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return ready_[ci] != 0; });
  }

 private:
  void work() {
    PlanScratch sx;
    for (;;) {
      const size_t ci = next_.fetch_add(1);
      if (ci >= cut_.chunks.size() || stop_.load()) return;
      plan_chunk(env_, cut_, cut_.chunks[ci], plan_, order_, sx);
      {
        std::lock_guard<std::mutex> g(mu_);
        ready_[ci] = 1;
      }
      cv_.notify_all();
    }
  }
  const PlanEnv &env_;
  BatchCut &cut_;
  PlanTask *plan_;
  int32_t *order_;
  WorkerPool *pool_;
  std::vector<char> ready_;
  size_t first_ = 0;
  std::atomic<size_t> next_{0};
  std::atomic<bool> stop_{false};
  std::mutex mu_;
  std::condition_variable cv_;
  PlanScratch own_;
};

}  // namespace

// One part of a batch call on one context: cut, plan and launch `n` tasks whose results go to d_out[0 .. n); nothing is
// waited for.  `n_scan`: the records the closing CIGAR scan of this context will cover (the whole call's, when this part
// closes it).  The caller closes the call with finish_batch.
static int batch_part(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, size_t n_scan, const uint32_t *d_pool,
                      uint32_t want, sdf_result *d_out, hipStream_t st, BatchRun &run) {
  ctx->err.clear();
  for (float &m : ctx->ms) m = 0.f;
  ctx->launches = 0;
  ctx->paired = 0;
  std::fill(ctx->tb_classes, ctx->tb_classes + 14, (int64_t)0);
  // (nothing of this context's earlier calls is in flight: what they outgrew is idle now -- sdf_ctx.h: DevBuf)
  for_each_device_buffer(ctx, [](DevBuf &b) { b.new_call(); }, BufGroup::BatchCall);
  const auto host_t0 = std::chrono::steady_clock::now();
  auto host_ms = [&] { return (float)ms_since(host_t0); };
  run.ctx = ctx;
  run.st = st;
  run.d_pool = d_pool;
  run.d_out = d_out;

  // ---- validate, cut into chunks ----
  if (int rc = make_scorek(ctx, sc, run.sk)) return rc;
  PlanEnv env = plan_env(ctx->cfg, sc, tasks, n, want, ctx->max_dyn_lds);
  env.lane_ok = env.lane_ok && ctx->pipeline_ok;  // (the lane kernel runs on a stream of its own)
  if (env.lane_ok) {
    SDF_HIP(ctx->host_lane.reserve(n * sizeof(LaneRec)));
    env.lane_recs = (LaneRec *)ctx->host_lane.p;
  }
  ctx->lane_tasks = 0;
  run.want_cigar = env.want_cigar();
  run.scoring = sc;
  run.tasks = tasks;
  run.want = want;
  ctx->reran = 0;
  if (!ctx->cut) ctx->cut = new BatchCut();
  BatchCut &cut = *ctx->cut;
  cut.reset();
  {
    // Planning threads of a context: SDF_PLAN_THREADS, else every CPU the process may use but this thread's when the
    // context is the only one of the process (the scan of a million tasks is CPU-bound: 1.7 ms on eight threads, 0.86 ms on
    // sixteen), seven when there are several (the stage driver's lanes share the machine).
    const int env_planners = (int)ctx->cfg.plan_threads;  // (-1: by the CPUs)
    // (one process per GPU: the ranks of a node share its CPUs -- LOCAL_WORLD_SIZE / WORLD_SIZE as torch.distributed sets them)
    static const int local_ranks = [] {
      const char *e = getenv("LOCAL_WORLD_SIZE");
      if (!e) e = getenv("WORLD_SIZE");
      return e ? std::max(1, atoi(e)) : 1;
    }();
    // (several contexts in one process AND several processes on the node -- bench.py's two calls in flight per rank: seven, or
    // the rank's share of the CPUs if that is less)
    const int share = std::max(1, std::min(15, usable_cpus() / local_ranks - 1));
    const int max_planners = env_planners >= 0 ? env_planners : g_live_contexts.load() > 1 ? std::min(7, share) : share;
    // (parked threads plan the chunks of batches of 120,000 tasks and more -- 250,000 tasks of the hg19 mixture:
    // 14.5 -> 10.1 ms, the headline batch unchanged -- and scan the cut as well: sdf_plan.hip, scan_from)
    const size_t pool_from = (size_t)ctx->cfg.plan_pool_from;
    if (!ctx->pool && n >= pool_from && max_planners > 0 && !ctx->is_part) ctx->pool = new WorkerPool(max_planners, (int)ctx->cfg.pool_spin_us);
  }
  run.cut = &cut;
  const bool dbg_plan_chunks = ctx->cfg.debug_plan != 0;

  // ---- buffers and the start of the call on the device: once with upper bounds, before the early start of the heavy
  // chunks (while the batch is still being read), and / or with the cut's sums ----
  bool begun = false;
  auto prepare = [&](const bool early) -> int {
    const size_t lane_need = cut.use_lane ? ((cut.lane_dir_bytes + 255) & ~(size_t)255) : 0;
    // (heavy tasks' slice first: it stays where it is when the workspace has to grow after the early start -- an
    // outgrown buffer is retired, not freed -- and the chunks launched by then keep their pointer)
    const size_t dir_bytes = early ? cut.heavy_need : cut.heavy_need + cut.region_need * cut.nreg_ws + lane_need;
    if (ctx->dir_ws.reserve(std::max<size_t>(dir_bytes, 256), ctx->ws_budget + 4096) != hipSuccess) {
      ctx->err = "cannot allocate the direction-matrix workspace";
      (void)hipGetLastError();
      return SDF_ERR_NOMEM;
    }
    const size_t n_lane = cut.use_lane ? cut.n_lane : 0;
    const size_t np = early ? n : std::max<size_t>(cut.ntask_total, 1);
    const size_t np_dev = early ? n : np + n_lane;
    const int64_t words = early ? cut.stage_upper : cut.stage_total + (cut.use_lane ? cut.lane_stage_words : 0);
    const size_t nord = early ? std::max<size_t>(cut.order_upper, 2) : std::max<size_t>(cut.order_total, 2);
    SDF_HIP(ctx->stage_ws.reserve((size_t)std::max<int64_t>(words, 4) * 4));
    SDF_HIP(ctx->plan_buf.reserve(np_dev * sizeof(PlanTask)));
    SDF_HIP(ctx->order_buf.reserve(nord * sizeof(int32_t)));
    SDF_HIP(ctx->misc_buf.reserve(SDF_MISC_PARTS * 8 + ((std::max(n, n_scan) + 1023) / 1024 + 1) * 8));
    SDF_HIP(ctx->host_plan.reserve(np * sizeof(PlanTask)));
    SDF_HIP(ctx->host_order.reserve(nord * sizeof(int32_t)));
    // (the plan records and the CIGAR staging of the chunks started early are read again at the end of the call -- the
    // traceback's counters, the compaction, a re-run of abandoned tasks: their buffers were sized by bounds that hold.  The
    // launch order is not: a chunk's segment is uploaded and read by its own launches only, and an outgrown buffer --
    // device or pinned -- stays alive until the context goes, so the order buffers may grow here.)
    if (begun && (run.plan != (PlanTask *)ctx->host_plan.p || run.d_plan != (PlanTask *)ctx->plan_buf.p ||
                  run.d_stage != (uint32_t *)ctx->stage_ws.p)) {
      ctx->err = "internal: a buffer sized by its upper bound had to grow after the early start";
      return SDF_ERR_INVALID;
    }
    run.plan = (PlanTask *)ctx->host_plan.p;  // pinned: the uploads are asynchronous
    run.order = (int32_t *)ctx->host_order.p;
    run.d_plan = (PlanTask *)ctx->plan_buf.p;
    run.d_order = (int32_t *)ctx->order_buf.p;
    run.d_dir = (uint8_t *)ctx->dir_ws.p;
    run.d_stage = (uint32_t *)ctx->stage_ws.p;
    if (!begun) {
      run.heavy_dir = run.d_dir;
      SDF_HIP(ctx->claim_buf.reserve(kClaimSets * 8 * sizeof(unsigned)));
      SDF_HIP(hipMemsetAsync(ctx->claim_buf.p, 0, kClaimSets * 8 * sizeof(unsigned), st));
      SDF_HIP(hipMemsetAsync((unsigned long long *)ctx->misc_buf.p + 1, 0, sizeof(unsigned long long), st));
      run.ev_begin = next_event(ctx, run.evc);
      hipLaunchKernelGGL(reset_results_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_out, (int)n);
      SDF_HIP(hipEventRecord(run.ev_begin, st));
      // (the internal streams are ordered behind ev_begin by launch_chunk, each before its first use in this call)
      begun = true;
    }
    return SDF_OK;
  };
  // the early start: plan and launch the heavy chunks (cut.chunks at that moment) on this thread
  PlanScratch early_scratch;
  const std::function<int()> early = [&]() -> int {
    if (int prc = prepare(true)) return prc;
    run.have_heavy = true;
    run.more_chunks = true;
    run.cev.assign(cut.chunks.size(), ChunkEv{});
    for (size_t ci = 0; ci < cut.chunks.size(); ++ci) {
      ChunkPlan &c = cut.chunks[ci];
      plan_chunk(env, cut, c, run.plan, run.order, early_scratch);
      if (ci == 0) ctx->ms[4] = host_ms();
      if (c.err) {
        ctx->err = c.err;
        return SDF_ERR_INVALID;
      }
      ctx->paired += c.paired;
      const float tw = host_ms();
      if (int lrc = launch_chunk(run, ci)) return lrc;
      if (dbg_plan_chunks) fprintf(stderr, "[chunk %zu: %zu tasks (heavy, early) planned by %.2f ms, launched by %.2f ms]\n", ci, c.cnt, tw, host_ms());
      cut.n_early = ci + 1;
    }
    return SDF_OK;
  };
  {
    const char *msg = nullptr;
    const bool early_on = ctx->cfg.early_heavy != 0;  // (0: the heavy chunks wait for the whole cut, as every other chunk)
    const int crc = cut_batch(env, ctx->pipeline_ok, ctx->ws_budget, cut, &msg, ctx->pool, early_on && !ctx->is_part ? &early : nullptr);
    run.more_chunks = false;
    if (crc) {
      if (ctx->err.empty()) ctx->err = msg ? msg : "invalid batch";
      if (begun) drain_streams(ctx, st);
      return crc;
    }
  }
  run.have_heavy = !cut.chunks.empty() && cut.chunks[0].heavy;
  const float dbg_a = host_ms();
  if (int prc = prepare(false)) {
    if (cut.n_early) drain_streams(ctx, st);
    return prc;
  }
  run.cev.resize(cut.chunks.size(), ChunkEv{});
  const float dbg_b = host_ms();
  if (cut.use_lane)
    if (int lrc = launch_lane(run, n)) {
      drain_streams(ctx, st);
      return lrc;
    }

  // ---- plan (worker threads, chunk order) and launch (this thread, chunk order) ----
  int rc = SDF_OK;
  float dbg_c = 0.f;
  {
    // (batches of ordinary size are planned by this thread, a chunk ahead of the GPU: 25,000 tasks take under a
    // millisecond to plan and five to run; batches of many small tasks are planned on the context's parked threads)
    const int nthr = ctx->pool && cut.chunks.size() >= 3
                         ? (int)std::min<size_t>(ctx->pool->size(), cut.chunks.size())
                         : 0;
    ChunkPlanner planner(env, cut, run.plan, run.order, ctx->pool, nthr, cut.n_early);
    dbg_c = host_ms();
    for (size_t ci = cut.n_early; ci < cut.chunks.size() && rc == SDF_OK; ++ci) {
      planner.wait(ci);
      if (ci == 0) ctx->ms[4] = host_ms();
      const ChunkPlan &c = cut.chunks[ci];
      if (c.err) {
        ctx->err = c.err;
        rc = SDF_ERR_INVALID;
        break;
      }
      ctx->paired += c.paired;
      const float tw = host_ms();
      rc = launch_chunk(run, ci);
      if (dbg_plan_chunks)
        fprintf(stderr, "[chunk %zu: %zu tasks%s planned by %.2f ms, launched by %.2f ms; flags %.3f GB placed in a region of %.3f GB (the bound)]\n", ci,
                c.cnt, c.heavy ? " (heavy)" : "", tw, host_ms(), (double)c.dir_bytes * 1e-9,
                (double)(c.heavy ? cut.heavy_need : cut.region_need) * 1e-9);
    }
  }
  if (rc != SDF_OK) {  // earlier chunks are in flight and reference the context's buffers: let them finish
    drain_streams(ctx, st);
    return rc;
  }
  if (ctx->cfg.debug_plan)
    fprintf(stderr, "[plan: n=%zu cut %.2f ms, buffers %.2f ms, planner up %.2f ms, first chunk planned %.2f ms, all launched %.2f ms; chunks %zu heavy %zu]\n", n,
            dbg_a, dbg_b, dbg_c, ctx->ms[4], host_ms(), cut.chunks.size(), cut.n_heavy);
  return SDF_OK;
}

extern "C" int sdf_extz2_batch_device(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks,
                                      size_t n, const uint32_t *d_pool, uint32_t want,
                                      sdf_result *d_out, uint32_t *d_cig, size_t cigar_cap,
                                      size_t *cigar_used, void *stream_) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const auto host_t0 = std::chrono::steady_clock::now();
  auto host_ms = [&] { return (float)ms_since(host_t0); };
  if (cigar_used) *cigar_used = 0;
  if (n == 0) return SDF_OK;
  if (!tasks || !d_out || n > 0x7fffffffu) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream_ ? (hipStream_t)stream_ : ctx->stream;
  const bool dbg_plan_chunks = ctx->cfg.debug_plan != 0;
  // SDF_SPLIT_MIN=<tasks>: a batch of that many tasks or more starts in two parts.  Everything the GPU waits for before
  // its first launch is a pass over the caller's task array (40 bytes per task: 1.6-3 ms for a million tasks on eight
  // threads); the first part -- an eighth of the tasks (SDF_SPLIT_DIV) -- is cut, planned and launched on a second context
  // of this device, on a thread of its own, while this thread reads the rest.  The parts write disjoint ranges of the
  // result array; the CIGAR scan and the compaction at the end cover both.  Measured on the 1,000,000-task hg19 mixture:
  // 16.5 ms against 17.2 ms on one box, 17.7 against 15.4 on another -- within the box-to-box noise, and a second set of
  // streams and buffers: off by default, kept under test (tests/test_gpu_extz2.py).
  // By default (end of round 3) batches of 50,000 to 400,000 tasks of one size (see uniform_mid) on a process's only context
  // start that way with a first part of 8,192 tasks: their cut is a pass on ONE thread (1 ms for the 100,000 tasks of the headline batch) that the
  // first launch no longer waits for -- 1,110 against 1,088-1,090 Gcell/s, three runs each on one box.  Larger batches
  // start their heavy chunks early instead (cut_batch's two passes); SDF_SPLIT_MIN=0 turns the split off.
  const long long split_env = (long long)ctx->cfg.split_min;  // (-1: the default rule; 0: off)
  const int split_div = (int)ctx->cfg.split_div;
  // (only batches of tasks of one size, none of them long or small, by a sample of 256: 8,192 of them must keep the device
  // busy for the millisecond the cut of the rest takes, and a second context's streams next to the many small launches of a
  // batch of mixed lengths cost more than the early start brings -- mm8-like mixed bands, 100,000 tasks: 585 ms against 441;
  // hg19-shaped 250,000: 7.8 against 7.3)
  auto uniform_mid = [&] {
    const size_t step = n / 256;
    int mn = 0x7fffffff, mx = 0;
    double cells = 0;
    for (size_t i = 0; i < 256; ++i) {
      const sdf_task &t = tasks[i * step];
      const int d = t.qlen + t.tlen;
      mn = std::min(mn, d);
      mx = std::max(mx, d);
      const double full = (double)t.qlen * t.tlen;
      cells += t.w < 0 ? full : std::min(full, (2.0 * t.w + 1) * std::min(t.qlen, t.tlen));
    }
    return mn > 0 && mx <= 2 * mn && mx <= 4096 && cells >= 256 * 1e5;
  };
  const bool split_default = split_env < 0 && n >= 50000 && n < 400000 && g_live_contexts.load() == 1 && uniform_mid();
  const bool split_asked = split_env > 0 && n >= (size_t)split_env;
  BatchRun run, first;
  BatchRun *head = nullptr;
  size_t n_first = 0;
  if (ctx->pipeline_ok && (split_default || split_asked) && !ctx->is_part) {
    if (!ctx->part_ctx) {
      sdf_config pc = ctx->cfg;  // (the parent's settings, whatever the environment says now)
      pc.workspace_gib = 0;
      pc.debug_plan = 0;
      ctx->part_ctx = sdf_create_cfg(ctx->device, ctx->ws_budget / 4, &pc);
      if (ctx->part_ctx) mark_internal_context(ctx->part_ctx);  // (a part context is not another user of the process's CPUs)
    }
    // (a batch of fewer than two blocks has no second part: SDF_SPLIT_MIN below 4,096 tasks would otherwise round the first
    // part up past the end of the batch -- ADVICE r3)
    size_t want_first = split_asked ? (n / split_div + SDF_CUT_BLOCK - 1) / SDF_CUT_BLOCK * SDF_CUT_BLOCK : 2 * SDF_CUT_BLOCK;
    if (n >= 2 * SDF_CUT_BLOCK && want_first + SDF_CUT_BLOCK > n) want_first = (n - SDF_CUT_BLOCK) / SDF_CUT_BLOCK * SDF_CUT_BLOCK;
    sdf_ctx *pc = n >= 2 * SDF_CUT_BLOCK && want_first >= SDF_CUT_BLOCK ? ctx->part_ctx : nullptr;
    if (pc) {
      n_first = want_first;
      // the part's stream starts where the caller's stream is
      if (ctx->part_ev == nullptr) (void)hipEventCreate(&ctx->part_ev);
      SDF_HIP(hipEventRecord(ctx->part_ev, st));
      SDF_HIP(hipStreamWaitEvent(pc->stream, ctx->part_ev, 0));
      head = &first;
    }
  }
  // (the first part on a thread of its own -- it plans on that thread alone, the planning threads are this part's --
  // while this thread reads the rest of the task array)
  int rc_first = SDF_OK;
  std::thread first_thread;
  if (head)
    first_thread = std::thread([&] {
      (void)hipSetDevice(ctx->device);
      rc_first = batch_part(ctx->part_ctx, sc, tasks, n_first, 0, d_pool, want, d_out, ctx->part_ctx->stream, first);
    });
  const int rc_main = batch_part(ctx, sc, tasks + n_first, n - n_first, n, d_pool, want, d_out + n_first, st, run);
  if (head) first_thread.join();
  if (rc_first != SDF_OK || rc_main != SDF_OK) {
    if (head) drain_streams(head->ctx, head->st);
    drain_streams(ctx, st);
    if (rc_main == SDF_OK) ctx->err = head->ctx->err;
    return rc_main != SDF_OK ? rc_main : rc_first;
  }
  int rc = finish_batch(run, head, n, d_out, d_cig, cigar_cap, cigar_used);
  if (rc != SDF_OK) {
    drain_streams(ctx, st);
    if (head) drain_streams(head->ctx, head->st);
    return rc;
  }
  if (head) {  // the call's statistics cover both parts
    ctx->launches += head->ctx->launches;
    ctx->paired += head->ctx->paired;
    ctx->lane_tasks += head->ctx->lane_tasks;
    ctx->reran += head->ctx->reran;
    for (int c = 0; c < 14; ++c) ctx->tb_classes[c] += head->ctx->tb_classes[c];
    ctx->ms[4] = head->ctx->ms[4];  // host time before the call's first launch
  }
  ctx->ms[5] = host_ms();
  if (dbg_plan_chunks) fprintf(stderr, "[batch finished by %.2f ms]\n", ctx->ms[5]);
  return SDF_OK;
}

__global__ void brief_results_kernel(const sdf_result *__restrict__ res, sdf_result_brief *__restrict__ out, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  sdf_result_brief b;
  b.cigar_off = res[k].cigar_off;
  b.n_cigar = (int32_t)res[k].n_cigar;
  b.matches = res[k].matches;
  out[k] = b;
}

// (view: the caller reads records and CIGAR words where the device's copies land -- the context's pinned staging, valid until
// the context's next call -- instead of receiving copies in arrays of its own)
struct ResultView {
  bool brief = true;
  const void *res = nullptr;
  const uint32_t *cig = nullptr;
};
static int batch_host_tail(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *t2, size_t n, size_t words, uint32_t want,
                           sdf_result *out, sdf_result_brief *brief, uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used,
                           int nthr, std::chrono::steady_clock::time_point dbg0, std::chrono::steady_clock::time_point dbg1,
                           const char *what, ResultView *view = nullptr);

// The host-buffer call: sequences packed into pinned memory, one upload, the device-resident call, results and CIGARs back
// through pinned staging.  `brief`: 16-byte records instead of sdf_result (sdf_extz2_batch_brief).
static int batch_host(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, const uint8_t *seq_pool,
                      size_t pool_bytes, uint32_t want, sdf_result *out, sdf_result_brief *brief, uint32_t *cigar_pool,
                      size_t cigar_cap, size_t *cigar_used) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (cigar_used) *cigar_used = 0;
  if (n == 0) return SDF_OK;
  if (!tasks || (!out && !brief) || (!seq_pool && pool_bytes)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  SDF_HIP(hipSetDevice(ctx->device));
  // pack every referenced sequence once (2-bit codes + N mask) and rewrite offsets to words
  const auto dbg0 = std::chrono::steady_clock::now();
  // (the task array with word offsets: kept by the context -- a fresh vector of 700,000 tasks is 34 MB of page faults per
  // call -- the offsets written here, the other fields copied by the packing threads below)
  std::vector<sdf_task> &t2 = ctx->host_tasks;
  if (t2.size() < n) t2.resize(n + n / 2);
  size_t words = 0;
  for (size_t k = 0; k < n; ++k) {
    const sdf_task &t = tasks[k];
    if (!in_range(t.q_off, t.qlen, pool_bytes) || !in_range(t.t_off, t.tlen, pool_bytes)) {
      ctx->err = "task sequence range outside the pool";
      return SDF_ERR_INVALID;
    }
    t2[k].q_off = (int64_t)words;
    words += sdf_packed_words(t.qlen);
    t2[k].t_off = (int64_t)words;
    words += sdf_packed_words(t.tlen);
  }
  // packed straight into pinned memory (the upload is then one asynchronous DMA), on a few threads when the batch is
  // large; results and CIGARs come back through pinned staging too (a pageable hipMemcpy runs at ~2.5 GB/s here)
  SDF_HIP(ctx->host_pool.reserve(std::max<size_t>(words, 1) * 4));
  uint32_t *packed = (uint32_t *)ctx->host_pool.p;
  auto pack_range = [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const int64_t qo = t2[k].q_off, to = t2[k].t_off;
      t2[k] = tasks[k];
      t2[k].q_off = qo;
      t2[k].t_off = to;
      if (tasks[k].qlen > 0) sdf_pack_codes(seq_pool + tasks[k].q_off, tasks[k].qlen, packed + t2[k].q_off);
      if (tasks[k].tlen > 0) sdf_pack_codes(seq_pool + tasks[k].t_off, tasks[k].tlen, packed + t2[k].t_off);
    }
  };
  // (at most four when the process has several contexts -- the stage driver runs up to three of these calls at once next to
  // its own worker threads --, eight for a process's only context)
  const unsigned thr_cap = g_live_contexts.load() > 1 ? 4u : (unsigned)std::max(1, std::min(8, usable_cpus() / 2));
  const int nthr = words >= (1u << 18) ? (int)std::min<unsigned>(thr_cap, std::max(1u, std::thread::hardware_concurrency())) : 1;
  {
    // equal shares of words, not of tasks
    std::vector<size_t> cut(nthr + 1, n);
    cut[0] = 0;
    for (int q = 1; q < nthr; ++q) {
      const int64_t target = (int64_t)(words * (size_t)q / (size_t)nthr);
      size_t lo = cut[q - 1], hi = n;
      while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (t2[mid].q_off < target) lo = mid + 1; else hi = mid;
      }
      cut[q] = lo;
    }
    std::vector<std::thread> thr;
    for (int q = 1; q < nthr; ++q) thr.emplace_back(pack_range, cut[q], cut[q + 1]);
    pack_range(cut[0], cut[1]);
    for (auto &th : thr) th.join();
  }
  const auto dbg1 = std::chrono::steady_clock::now();
  SDF_HIP(ctx->h_pool.reserve(std::max<size_t>(words, 1) * 4));
  SDF_HIP(hipMemcpyAsync(ctx->h_pool.p, packed, std::max<size_t>(words, 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  return batch_host_tail(ctx, sc, t2.data(), n, words, want, out, brief, cigar_pool, cigar_cap, cigar_used, nthr, dbg0, dbg1, "sdf_extz2_batch");
}

// ... the rest of a host-buffer call once the packed sequences are (being) written to ctx->h_pool on ctx->stream: the
// device-resident call, results and CIGAR words back through pinned staging.
static int batch_host_tail(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *t2, size_t n, size_t words, uint32_t want,
                           sdf_result *out, sdf_result_brief *brief, uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used,
                           int nthr, std::chrono::steady_clock::time_point dbg0, std::chrono::steady_clock::time_point dbg1,
                           const char *what, ResultView *view) {
  const bool dbg_t = ctx->cfg.debug_timing != 0;
  SDF_HIP(ctx->h_out.reserve(n * sizeof(sdf_result)));
  SDF_HIP(ctx->h_cig.reserve(std::max<size_t>(cigar_cap, 1) * 4));
  size_t used = 0;
  int rc = sdf_extz2_batch_device(ctx, sc, t2, n, (const uint32_t *)ctx->h_pool.p, want,
                                  (sdf_result *)ctx->h_out.p, (uint32_t *)ctx->h_cig.p, cigar_cap, &used,
                                  ctx->stream);
  if (cigar_used) *cigar_used = used;
  if (rc != SDF_OK) return rc;
  const auto dbg2 = std::chrono::steady_clock::now();
  const bool as_brief = view ? view->brief : brief != nullptr;
  const size_t out_bytes = n * (as_brief ? sizeof(sdf_result_brief) : sizeof(sdf_result)), cig_bytes = (used && (cigar_pool || view)) ? used * 4 : 0;
  SDF_HIP(ctx->host_out.reserve(out_bytes + cig_bytes + 64));
  uint8_t *stg = (uint8_t *)ctx->host_out.p;
  const void *d_res = ctx->h_out.p;
  if (as_brief) {
    SDF_HIP(ctx->h_brief.reserve(out_bytes));
    hipLaunchKernelGGL(brief_results_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const sdf_result *)ctx->h_out.p, (sdf_result_brief *)ctx->h_brief.p, (int)n);
    d_res = ctx->h_brief.p;
  }
  void *const out_any = brief ? (void *)brief : (void *)out;
  SDF_HIP(hipMemcpyAsync(stg, d_res, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (cig_bytes) SDF_HIP(hipMemcpyAsync(stg + out_bytes, ctx->h_cig.p, cig_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SDF_HIP(hipStreamSynchronize(ctx->stream));
  if (view) {
    view->res = stg;
    view->cig = (const uint32_t *)(stg + out_bytes);
  } else {
    auto copy_range = [&](int q, int of) {
      const size_t a = out_bytes * (size_t)q / (size_t)of, b = out_bytes * (size_t)(q + 1) / (size_t)of;
      memcpy((uint8_t *)out_any + a, stg + a, b - a);
      const size_t c = cig_bytes * (size_t)q / (size_t)of, d = cig_bytes * (size_t)(q + 1) / (size_t)of;
      if (d > c) memcpy((uint8_t *)cigar_pool + c, stg + out_bytes + c, d - c);
    };
    const int nc = out_bytes + cig_bytes >= (8u << 20) ? std::min(nthr > 1 ? nthr : 4, 4) : 1;
    std::vector<std::thread> thr;
    for (int q = 1; q < nc; ++q) thr.emplace_back(copy_range, q, nc);
    copy_range(0, nc);
    for (auto &th : thr) th.join();
  }
  if (dbg_t) {
    const auto dbg3 = std::chrono::steady_clock::now();
    fprintf(stderr, "[%s n=%zu words=%zu cap=%zu used=%zu] pack %.1f ms, h2d+device %.1f ms (plan %.1f, dp %.1f, tb %.1f), d2h %.1f ms%s\n",
            what, n, words, cigar_cap, used, ms_between(dbg0, dbg1), ms_between(dbg1, dbg2), ctx->ms[4], ctx->ms[0], ctx->ms[1], ms_between(dbg2, dbg3),
            ctx->reran ? (", " + std::to_string(ctx->reran) + " tasks given up by a stripe wait and run again").c_str() : "");
  }
  return SDF_OK;
}

extern "C" int sdf_extz2_batch(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                               const uint8_t *seq_pool, size_t pool_bytes, uint32_t want,
                               sdf_result *out, uint32_t *cigar_pool, size_t cigar_cap,
                               size_t *cigar_used) {
  return batch_host(ctx, sc, tasks, n, seq_pool, pool_bytes, want, out, nullptr, cigar_pool, cigar_cap, cigar_used);
}

extern "C" int sdf_extz2_batch_brief(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                                     const uint8_t *seq_pool, size_t pool_bytes, sdf_result_brief *out,
                                     uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used) {
  return batch_host(ctx, sc, tasks, n, seq_pool, pool_bytes, SDF_WANT_CIGAR | SDF_WANT_SCORE, nullptr, out, cigar_pool, cigar_cap,
                    cigar_used);
}

// The strand bits of a resident task (include/sedef_hip.h) are consumed where characters become codes (seq_pack.hip): this is
// the flag word the planner gets.  Every other entry point hands its flags over as they are, where the bits are unknown ones.
constexpr int32_t kStrandBits = SDF_TASK_Q_RC | SDF_TASK_T_RC;
static inline int32_t planner_flag(int32_t flag) { return flag & ~kStrandBits; }

static int batch_pairs(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want, sdf_result *out,
                       sdf_result_brief *brief, uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used,
                       ResultView *view = nullptr) {
  using sdf::PackRec;
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (cigar_used) *cigar_used = 0;
  if (n == 0) return SDF_OK;
  if (!tasks || (!out && !brief && !view) || n > 0x3fffffffu) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  SDF_HIP(hipSetDevice(ctx->device));
  const auto dbg0 = std::chrono::steady_clock::now();
  // The task array with WORD offsets for the planner and the kernels, and one 32-byte record per task for the packing
  // kernel: where the task's characters are and where its packed words go.  Two passes over blocks of tasks on a few
  // threads (700,000 tasks a round in the chr1-sized stage run): the words of each block, then the records.
  std::vector<sdf_task> &t2 = ctx->host_tasks;
  if (t2.size() < n) t2.resize(n + n / 2);
  SDF_HIP(ctx->host_pool.reserve(n * sizeof(PackRec)));
  PackRec *recs = (PackRec *)ctx->host_pool.p;
  const size_t block = 32768, nb = (n + block - 1) / block, pool_bytes = ctx->pool_bytes;
  std::vector<size_t> bwords(nb + 1, 0), bcap(nb, 0);
  std::atomic<bool> bad(false), any_rc(false);
  const unsigned thr_cap = g_live_contexts.load() > 1 ? 4u : (unsigned)std::max(1, std::min(8, usable_cpus() / 2));
  const int nthr = (int)std::min<size_t>(nb, thr_cap);
  auto on_blocks = [&](const std::function<void(size_t)> &f) {
    std::atomic<size_t> next(0);
    auto work = [&] {
      for (size_t b = next.fetch_add(1); b < nb; b = next.fetch_add(1)) f(b);
    };
    std::vector<std::thread> thr;
    for (int q = 1; q < nthr; ++q) thr.emplace_back(work);
    work();
    for (auto &th : thr) th.join();
  };
  on_blocks([&](size_t b) {
    size_t w = 0, c = 0;
    for (size_t k = b * block; k < std::min(n, (b + 1) * block); ++k) {
      const sdf_task &t = tasks[k];
      if (!in_range(t.q_off, t.qlen, pool_bytes) || !in_range(t.t_off, t.tlen, pool_bytes)) bad.store(true);
      w += sdf_packed_words(t.qlen) + sdf_packed_words(t.tlen);
      c += (size_t)t.qlen + (size_t)t.tlen + 2;
    }
    bwords[b + 1] = w;
    bcap[b] = c;
  });
  if (view) {  // (no caller's pool to fit: the staging takes the words there are; the device's bound is the worst case)
    cigar_cap = 16;
    for (size_t b = 0; b < nb; ++b) cigar_cap += bcap[b];
  }
  if (bad.load()) {
    ctx->err = "task sequence range outside the resident pool (sdf_pool_upload)";
    return SDF_ERR_INVALID;
  }
  for (size_t b = 0; b < nb; ++b) bwords[b + 1] += bwords[b];
  const size_t words = bwords[nb];
  on_blocks([&](size_t b) {
    size_t w = bwords[b];
    int32_t block_rc = 0;  // (one store per block: the threads share the flag's cache line)
    for (size_t k = b * block; k < std::min(n, (b + 1) * block); ++k) {
      const sdf_task &t = tasks[k];
      PackRec &r = recs[k];
      r.q_byte = t.q_off;
      r.t_byte = t.t_off;
      r.q_word = (int64_t)w;
      r.qlen = (int32_t)((uint32_t)t.qlen | ((t.flag & SDF_TASK_Q_RC) ? sdf::kPackRc : 0u));
      r.tlen = (int32_t)((uint32_t)t.tlen | ((t.flag & SDF_TASK_T_RC) ? sdf::kPackRc : 0u));
      block_rc |= t.flag;
      t2[k] = t;
      t2[k].flag = planner_flag(t.flag);  // (the strand is the packing's alone: the planner and the DP kernels never see it)
      t2[k].q_off = (int64_t)w;
      w += sdf_packed_words(t.qlen);
      t2[k].t_off = (int64_t)w;
      w += sdf_packed_words(t.tlen);
    }
    if (block_rc & kStrandBits) any_rc.store(true, std::memory_order_relaxed);
  });
  const auto dbg1 = std::chrono::steady_clock::now();
  for_each_device_buffer(ctx, [](DevBuf &b) { b.new_call(); }, BufGroup::Pairs);
  SDF_HIP(ctx->h_pool.reserve(std::max<size_t>(words, 1) * 4));
  SDF_HIP(ctx->pk_recs.reserve(n * sizeof(PackRec)));
  SDF_HIP(hipMemcpyAsync(ctx->pk_recs.p, recs, n * sizeof(PackRec), hipMemcpyHostToDevice, ctx->stream));
  // (a batch without a reversed side -- every batch of the stage driver -- runs the forward-only kernel)
  hipLaunchKernelGGL(any_rc.load() ? sdf::pack_chars_kernel<true> : sdf::pack_chars_kernel<false>, dim3((unsigned)((2 * n + 15) / 16)),
                     dim3(256), 0, ctx->stream, (const PackRec *)ctx->pk_recs.p, (long long)(2 * n), (const char *)ctx->an_pool.p,
                     (uint32_t *)ctx->h_pool.p);
  return batch_host_tail(ctx, sc, t2.data(), n, words, want, out, brief, cigar_pool, cigar_cap, cigar_used, nthr, dbg0, dbg1,
                         "sdf_extz2_batch_pairs", view);
}

extern "C" int sdf_extz2_batch_pairs_view(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                                          const sdf_result_brief **out, const uint32_t **cigar_pool, size_t *cigar_used) {
  if (!out || !cigar_pool) return SDF_ERR_INVALID;
  *out = nullptr;
  *cigar_pool = nullptr;
  ResultView v;
  const int rc = batch_pairs(ctx, sc, tasks, n, SDF_WANT_CIGAR | SDF_WANT_SCORE, nullptr, nullptr, nullptr, 0, cigar_used, &v);
  if (rc == SDF_OK) {
    *out = (const sdf_result_brief *)v.res;
    *cigar_pool = v.cig;
  }
  return rc;
}

extern "C" int sdf_extz2_batch_pairs(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, sdf_result_brief *out,
                                     uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used) {
  return batch_pairs(ctx, sc, tasks, n, SDF_WANT_CIGAR | SDF_WANT_SCORE, nullptr, out, cigar_pool, cigar_cap, cigar_used);
}

extern "C" int sdf_extz2_batch_pairs_full(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want,
                                          sdf_result *out, uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used) {
  return batch_pairs(ctx, sc, tasks, n, want, out, nullptr, cigar_pool, cigar_cap, cigar_used);
}

// ---- one-task drop-in with the reference's exact signature (extern/ksw2.h:50) -----------------
namespace {
std::mutex g_mu;
sdf_ctx *g_ctx = nullptr;
}  // namespace

extern "C" void sdf_ksw_extz2(void * /*km*/, int qlen, const uint8_t *query, int tlen,
                              const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e,
                              int w, int zdrop, int flag, sdf_ksw_extz_t *ez) {
  ez->max_q = ez->max_t = ez->mqe_t = ez->mte_q = -1;
  ez->max = 0;
  ez->score = ez->mqe = ez->mte = SDF_NEG_INF;
  ez->n_cigar = 0;
  ez->m_cigar = 0;
  ez->zdropped = 0;
  ez->cigar = 0;
  if (m <= 0 || qlen <= 0 || tlen <= 0) return;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_ctx) {
    const char *dv = getenv("SDF_DEVICE");
    g_ctx = sdf_create(dv ? atoi(dv) : 0, (size_t)1 << 30);
    if (!g_ctx) {
      fprintf(stderr, "sdf_ksw_extz2: %s\n", sdf_last_error(nullptr));
      exit(120);
    }
  }
  sdf_scoring sc;
  memset(&sc, 0, sizeof(sc));
  sc.m = m;
  if (m == 5) memcpy(sc.mat, mat, 25);
  sc.gapo = q;
  sc.gape = e;
  std::vector<uint8_t> pool((size_t)qlen + tlen);
  memcpy(pool.data(), query, qlen);
  memcpy(pool.data() + qlen, target, tlen);
  sdf_task t;
  memset(&t, 0, sizeof(t));
  t.q_off = 0;
  t.t_off = qlen;
  t.qlen = qlen;
  t.tlen = tlen;
  t.w = w;
  t.zdrop = zdrop;
  t.flag = flag;
  sdf_result r;
  const size_t cap = (size_t)qlen + tlen + 2;
  uint32_t *cig = (uint32_t *)malloc(cap * 4);
  size_t used = 0;
  uint32_t want = SDF_WANT_ALL;
  if (flag & SDF_FLAG_SCORE_ONLY) want &= ~SDF_WANT_CIGAR;
  int rc = sdf_extz2_batch(g_ctx, &sc, &t, 1, pool.data(), pool.size(), want, &r, cig, cap, &used);
  if (rc != SDF_OK) {
    fprintf(stderr, "sdf_ksw_extz2: %s (rc=%d)\n", sdf_last_error(g_ctx), rc);
    exit(120);
  }
  ez->max = (uint32_t)r.max;
  ez->zdropped = (uint32_t)r.zdropped;
  ez->max_q = r.max_q;
  ez->max_t = r.max_t;
  ez->mqe = r.mqe;
  ez->mqe_t = r.mqe_t;
  ez->mte = r.mte;
  ez->mte_q = r.mte_q;
  ez->score = r.score;
  ez->n_cigar = r.n_cigar;
  if (r.n_cigar > 0) {
    ez->cigar = cig;
    ez->m_cigar = (int64_t)cap;
    if (r.cigar_off) memmove(cig, cig + r.cigar_off, (size_t)r.n_cigar * 4);
  } else {
    free(cig);
  }
}

// ---- planner without a device (not part of the public header; tests/test_planner.py, tests/test_plan_same.py) ------
// Cuts and plans a batch exactly like sdf_extz2_batch_device does (same code, same settings -- the environment's, like a
// context made now would get --, same thread pool).  The lane kernel's records need a device: `with_lane` gives the scan a
// host array for them instead (PlanEnv::lane_recs; lane_ok as plan_env sets it), so that the lane branch of the scan and
// the re-accounting of too few lane tasks are planned as well.
namespace {
struct DebugPlan {
  sdf_config cfg;
  std::vector<sdf_task> handed;
  std::vector<LaneRec> lane_recs;
  PlanEnv env;
  BatchCut cut;
  std::vector<PlanTask> plan;
  std::vector<int32_t> order;
  double ms = 0;  // cut + chunk planning
};

int debug_plan_run(DebugPlan &d, const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want, size_t ws_budget,
                   int max_dyn_lds, int nthreads, bool with_lane) {
  sdf_config &dcfg = d.cfg;
  {
    char why[256];
    if (sdf_config_from_env(&dcfg, why, sizeof why) != SDF_OK) return SDF_ERR_INVALID;
  }
  sdf_ctx tmp;  // only err is used: no HIP call is made here
  ScoreK sk;
  if (int rc = make_scorek(&tmp, sc, sk)) return rc;
  // Tasks as sdf_extz2_batch_pairs takes them may carry strand bits: the planner gets the flag word that call hands over
  std::vector<sdf_task> &handed = d.handed;
  for (size_t k = 0; k < n; ++k)
    if (tasks[k].flag & kStrandBits) {
      handed.assign(tasks, tasks + n);
      for (sdf_task &t : handed) t.flag = planner_flag(t.flag);
      tasks = handed.data();
      break;
    }
  d.env = plan_env(dcfg, sc, tasks, n, want, max_dyn_lds);
  if (with_lane && d.env.lane_ok) {
    d.lane_recs.assign(n, LaneRec());
    d.env.lane_recs = d.lane_recs.data();
  }
  const PlanEnv &env = d.env;
  BatchCut &cut = d.cut;
  const char *msg = nullptr;
  const auto tc0 = std::chrono::steady_clock::now();
  std::vector<PlanTask> &plan = d.plan;
  std::vector<int32_t> &order = d.order;
  // SDF_DEBUG_PLAN_EARLY=1: the cut in two passes with the early start of the heavy chunks (batch_part's, minus the
  // device): buffers by their upper bounds, the heavy chunks planned from the callback
  PlanScratch early_scratch;
  const std::function<int()> early = [&]() -> int {
    plan.resize(std::max<size_t>(n, 1));
    order.resize(std::max<size_t>(cut.order_upper, 2));
    for (size_t ci = 0; ci < cut.chunks.size(); ++ci) {
      plan_chunk(env, cut, cut.chunks[ci], plan.data(), order.data(), early_scratch);
      if (cut.chunks[ci].err) return SDF_ERR_INVALID;
      cut.n_early = ci + 1;
    }
    return SDF_OK;
  };
  {
    WorkerPool cut_pool(std::max(nthreads, 1));
    if (int rc = cut_batch(env, true, ws_budget, cut, &msg, nthreads > 0 ? &cut_pool : nullptr,
                           dcfg.debug_plan_early ? &early : nullptr))
      return rc;
  }
  if (dcfg.debug_plan)
    fprintf(stderr, "[sdf] debug plan: cut %.2f ms (%zu tasks, %d threads, %zu chunks started early)\n",
            ms_since(tc0), n, nthreads, cut.n_early);
  const size_t np = std::max<size_t>(cut.ntask_total, 1);
  if (cut.n_early && np > plan.size()) return SDF_ERR_INVALID;  // (the upper bound of the plan records holds)
  if (!cut.n_early) plan.resize(np);
  if (order.size() < std::max<size_t>(cut.order_total, 2)) order.resize(std::max<size_t>(cut.order_total, 2));
  {
    WorkerPool pool(std::max(nthreads, 1));
    ChunkPlanner planner(env, cut, plan.data(), order.data(), &pool, nthreads, cut.n_early);
    for (size_t ci = cut.n_early; ci < cut.chunks.size(); ++ci) planner.wait(ci);
  }
  d.ms = ms_since(tc0);
  for (const ChunkPlan &c : cut.chunks)
    if (c.err) return SDF_ERR_INVALID;
  return SDF_OK;
}
}  // namespace

// Reports, per input task: chunk index (-1: not run), launch class (LaunchClass::code), nreg, kind (TaskKind), dir_off,
// cig_slot, partner (index of the task it shares a wavefront with, -1 none), and per chunk {heavy, tasks, launches,
// dir_bytes, region capacity}.  No lane kernel.
extern "C" int sdf_debug_plan(const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want, size_t ws_budget,
                              int max_dyn_lds, int nthreads, int64_t *per_task /* n x 7 */, int64_t *per_chunk /* cap x 5 */,
                              size_t chunk_cap, size_t *nchunks) {
  DebugPlan d;
  if (int rc = debug_plan_run(d, sc, tasks, n, want, ws_budget, max_dyn_lds, nthreads, false)) return rc;
  const BatchCut &cut = d.cut;
  const std::vector<PlanTask> &plan = d.plan;
  const std::vector<int32_t> &order = d.order;
  for (size_t k = 0; k < n * 7; ++k) per_task[k] = -1;
  *nchunks = cut.chunks.size();
  for (size_t ci = 0; ci < cut.chunks.size(); ++ci) {
    const ChunkPlan &c = cut.chunks[ci];
    if (ci < chunk_cap) {
      int64_t *o = per_chunk + 5 * ci;
      o[0] = c.heavy;
      o[1] = (int64_t)c.cnt;
      o[2] = (int64_t)c.launches.size();
      o[3] = (int64_t)c.dir_bytes;
      o[4] = (int64_t)(c.heavy ? cut.heavy_need : cut.region_need);
    }
    for (const Launch &L : c.launches) {
      const bool pair = L.lc.two_per_entry();
      const bool chained = L.lc.fam == LaunchClass::Family::Chain;  // (an entry per block of a pair of tasks: the listed one's partner through zdrop)
      const bool stripes = L.lc.per_stripe();
      for (size_t e = 0; e < L.cnt; ++e) {
        int32_t rel = order[c.ob + L.off + e];
        if (stripes) {  // one entry per stripe: the task is reported at its stripe 0
          if ((uint32_t)rel >> 24) continue;
          rel &= 0xffffff;
        }
        for (int side = 0; side < (chained ? 2 : 1); ++side) {
          const PlanTask &lead = plan[c.pb + rel];
          if (side && lead.zdrop == rel) break;  // (a chain without a partner)
          const PlanTask &p = side ? plan[c.pb + lead.zdrop] : lead;
          int64_t *o = per_task + 7 * (size_t)p.out_idx;
          if (o[0] >= 0 && !(pair && o[6] == p.out_idx)) return SDF_ERR_INVALID;  // listed twice (only a self-pair may be)
          o[0] = (int64_t)ci;
          o[1] = L.lc.code();
          o[2] = p.nreg;
          o[3] = p.kind;
          o[4] = p.dir_off;
          o[5] = p.cig_slot;
          o[6] = pair ? plan[c.pb + order[c.ob + L.off + (e ^ 1)]].out_idx : chained ? plan[c.pb + p.zdrop].out_idx : -1;
        }
      }
    }
  }
  return SDF_OK;
}

// The whole plan, as the launcher reads it, in six digests: [0] the cut's figures with heavy_idx and the runnable tasks'
// bound[] and cap[], [1] every PlanTask field by field, [2] order[0 .. order_total), [3] the chunks, [4] their launches,
// [5] the lane figures, lane[] and the lane records.  `dump_path` (optional): every word that goes into the digests, in
// that order, as 64-bit words into a file -- to find where two plans part.  `plan_ms` (optional): cut + chunk planning.
extern "C" int sdf_debug_plan_dump(const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want, size_t ws_budget,
                                   int max_dyn_lds, int nthreads, int with_lane, uint64_t *digest /* 6 */,
                                   const char *dump_path, double *plan_ms) {
  DebugPlan d;
  if (int rc = debug_plan_run(d, sc, tasks, n, want, ws_budget, max_dyn_lds, nthreads, with_lane != 0)) return rc;
  if (plan_ms) *plan_ms = d.ms;
  const BatchCut &cut = d.cut;
  if (cut.bound.size() < n || cut.cap.size() < n || d.order.size() < cut.order_total) return SDF_ERR_INVALID;
  FILE *f = dump_path ? fopen(dump_path, "wb") : nullptr;
  if (dump_path && !f) return SDF_ERR_INVALID;
  uint64_t h = 0;
  auto add = [&](uint64_t v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    if (f) fwrite(&v, 8, 1, f);
  };
  auto close = [&](int section) {
    digest[section] = h;
    h = (uint64_t)section + 1;
    add(~0ull);  // (dump: a section mark)
  };
  for (uint64_t v : {(uint64_t)cut.pipelined, (uint64_t)cut.split_heavy, (uint64_t)cut.nch, (uint64_t)cut.max_regions,
                     (uint64_t)cut.nreg_ws, (uint64_t)cut.n_heavy, (uint64_t)cut.region_need, (uint64_t)cut.heavy_need,
                     (uint64_t)cut.stage_total, (uint64_t)cut.ntask_total, (uint64_t)cut.order_total, (uint64_t)cut.stage_upper,
                     (uint64_t)cut.order_upper, (uint64_t)cut.n_early, (uint64_t)cut.chunks.size(), (uint64_t)cut.heavy_idx.size()})
    add(v);
  for (uint32_t k : cut.heavy_idx) add(k);
  for (uint8_t b : cut.heavy) add(b);
  for (size_t k = 0; k < n; ++k)
    if (plan_detail::task_runs(d.env.tasks[k], d.env.degenerate)) add(((uint64_t)cut.bound[k] << 32) | cut.cap[k]);
  close(0);
  for (const ChunkPlan &c : cut.chunks) {
    if (c.pb + c.cnt > d.plan.size()) return SDF_ERR_INVALID;
    for (size_t k = 0; k < c.cnt; ++k) {
      const PlanTask &p = d.plan[c.pb + k];
      for (int64_t v : {p.q_word, p.t_word, p.dir_off, p.cig_slot, (int64_t)p.qlen, (int64_t)p.tlen, (int64_t)p.w, (int64_t)p.zdrop,
                        (int64_t)p.flag, (int64_t)p.ncol16, (int64_t)p.out_idx, (int64_t)p.cig_cap, (int64_t)p.nreg, (int64_t)p.kind})
        add((uint64_t)v);
    }
  }
  close(1);
  for (size_t k = 0; k < cut.order_total; ++k) add((uint32_t)d.order[k]);
  close(2);
  for (const ChunkPlan &c : cut.chunks)
    for (uint64_t v : {(uint64_t)c.s, (uint64_t)c.e, (uint64_t)c.heavy, (uint64_t)c.pb, (uint64_t)c.ob, (uint64_t)c.order_cap,
                       (uint64_t)c.stage0, (uint64_t)c.ntask, (uint64_t)c.stage_words, (uint64_t)c.cnt, (uint64_t)c.nord,
                       (uint64_t)c.layouts, (uint64_t)c.paired, (uint64_t)c.dir_bytes, (uint64_t)c.launches.size()})
      add(v);
  close(3);
  for (const ChunkPlan &c : cut.chunks)
    for (const Launch &L : c.launches) {
      uint64_t est;
      memcpy(&est, &L.est, 8);
      for (uint64_t v : {(uint64_t)L.lc.fam, (uint64_t)L.lc.nreg, (uint64_t)L.lc.stream, (uint64_t)L.lc.block, (uint64_t)L.lds,
                         (uint64_t)L.off, (uint64_t)L.cnt, (uint64_t)(int64_t)L.rmax, est})
        add(v);
    }
  close(4);
  for (uint64_t v : {(uint64_t)cut.use_lane, (uint64_t)cut.n_lane, (uint64_t)cut.lane_cls[0], (uint64_t)cut.lane_cls[1],
                     (uint64_t)cut.lane_cls[2], (uint64_t)cut.lane_cls[3], (uint64_t)cut.lane_stage_words, (uint64_t)cut.lane_dir_bytes})
    add(v);
  for (size_t k = 0; k < std::min(n, cut.lane.size()); ++k) add(cut.lane[k]);
  for (const LaneRec &r : d.lane_recs)
    for (uint64_t v : {(uint64_t)r.q_word, (uint64_t)r.t_word, (uint64_t)r.out_idx, (uint64_t)r.qlen_m1, (uint64_t)r.tlen_m1, (uint64_t)r.flag})
      add(v);
  close(5);
  if (f) fclose(f);
  return SDF_OK;
}

// ---- debugging aid (not part of the public header): copy the head of the direction workspace ----
extern "C" int sdf_debug_copy_dir(sdf_ctx *ctx, void *host, size_t bytes) {
  if (!ctx || !ctx->dir_ws.p) return SDF_ERR_INVALID;
  if (bytes > ctx->dir_ws.cap) bytes = ctx->dir_ws.cap;
  return hipMemcpy(host, ctx->dir_ws.p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? SDF_OK : SDF_ERR_HIP;
}
