// A context's lifecycle (include/sedef_hip.h): sdf_create / sdf_destroy, sdf_reserve, what a context holds and what its last
// call did.  What must visit every buffer or every stream of a context goes through the tables of sdf_ctx.h.
#include <hip/hip_runtime.h>

#include <sched.h>

#include <hipcub/hipcub.hpp>

#include "sdf_batch.h"
#include "stripe_sync.h"

using namespace sdf;

static std::string g_err;  // error of the last failed sdf_create

extern "C" int sdf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" const char *sdf_last_error(const sdf_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_err.c_str();
}

std::atomic<int> g_live_contexts{0};
// CPUs this process may really use: the affinity mask capped by the cgroup's CPU quota
int usable_cpus() {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n > 0 ? n : CPU_COUNT(&set), CPU_COUNT(&set));
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
    char q[32];
    long period = 0;
    if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
      n = std::min(n, (int)((atol(q) + period / 2) / period));
    fclose(f);
  }
  return std::max(n, 1);
}

extern "C" const sdf_config *sdf_get_config(const sdf_ctx *ctx) { return ctx ? &ctx->cfg : nullptr; }

extern "C" sdf_ctx *sdf_create(int device, size_t workspace_bytes) { return sdf_create_cfg(device, workspace_bytes, nullptr); }

extern "C" sdf_ctx *sdf_create_cfg(int device, size_t workspace_bytes, const sdf_config *cfg_in) {
  return create_context(device, workspace_bytes, cfg_in, true);
}

sdf_ctx *create_context(int device, size_t workspace_bytes, const sdf_config *cfg_in, bool pipeline_streams) {
  sdf_config cfg;
  if (cfg_in) {
    if (cfg_in->size != sizeof(sdf_config)) {
      g_err = "sdf_create_cfg: the configuration was not initialised by sdf_config_default / sdf_config_from_env (size field)";
      return nullptr;
    }
    cfg = *cfg_in;
  } else {
    char why[256];
    if (sdf_config_from_env(&cfg, why, sizeof why) != SDF_OK) {  // (a typo in an SDF_* variable is an error, not a silent default)
      g_err = std::string("environment: ") + why;
      return nullptr;
    }
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_err = "no HIP device available (this library has no CPU fallback)";
    return nullptr;
  }
  if (device < 0 || device >= n) {
    g_err = "device ordinal out of range";
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_err = "hipSetDevice failed";
    return nullptr;
  }
  Lap lap{cfg.debug_timing != 0, "[sdf_create %s at %.1f ms]\n"};
  sdf_ctx *ctx = new sdf_ctx();
  ctx->device = device;
  ctx->cfg = cfg;
  ctx->pipeline_ok = cfg.pipeline != 0;
  if (cfg.debug_timing) g_debug_timing.store(true, std::memory_order_relaxed);
  if (cfg.debug_plan) {
    std::string dump(sdf_config_dump(&cfg, nullptr, 0), '\0');
    sdf_config_dump(&cfg, &dump[0], dump.size());
    fprintf(stderr, "[sdf_create device %d: configuration]\n%s", device, dump.c_str());
  }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    g_err = "hipStreamCreate failed";
    delete ctx;
    return nullptr;
  }
  lap.at("first stream");
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  lap.at("mem info");
  // (0: half of the free HBM -- the workspace is allocated by NEED, region by region (cut_batch), so a large budget costs a
  // small batch nothing, and a batch of long banded tasks -- BASELINE configs[4] at 100,000 tasks: 131 GB of flags -- is not cut
  // into more, smaller chunks because of a constructor default: 64 GiB until round 4, 252 ms against 201 at 128 GiB)
  size_t budget = workspace_bytes ? workspace_bytes : free_b ? free_b / 2 : (size_t)64 << 30;
  if (cfg.workspace_gib > 0) budget = (size_t)(cfg.workspace_gib * 1073741824.0);  // (overrides the caller's figure: experiments with the stage driver)
  if (free_b && budget > free_b / 2) budget = free_b / 2;
  ctx->ws_budget = budget;
  // Every kernel that takes dynamic LDS may have up to 160 KiB of it.  The first five, the general kernel's LDS-resident
  // instantiations, decide what the planner may ask for: max_dyn_lds is raised only when all of them accept it.
  const int want_lds = 160 * 1024;
#define SDF_K(...) reinterpret_cast<const void *>(&__VA_ARGS__)
  const void *const dyn_lds_kernels[] = {
      SDF_K(extz2_general_kernel<64, false, false>), SDF_K(extz2_general_kernel<256, false, false>),
      SDF_K(extz2_general_kernel<1024, false, false>), SDF_K(extz2_general_kernel<1024, false, true>),
      SDF_K(extz2_general_kernel<256, false, true>),
      SDF_K(extz2_wave_kernel<1, false>), SDF_K(extz2_wave_kernel<1, true>), SDF_K(extz2_wave_kernel<2, false>),
      SDF_K(extz2_wave_kernel<2, true>), SDF_K(extz2_wave_kernel<3, false>), SDF_K(extz2_wave_kernel<3, true>),
      SDF_K(extz2_wave_kernel<6, false>), SDF_K(extz2_wave_kernel<6, true>), SDF_K(extz2_wave_kernel<4, false>),
      SDF_K(extz2_wave_kernel<4, true>), SDF_K(extz2_wave_kernel<8, false>), SDF_K(extz2_wave_kernel<8, true>),
      SDF_K(extz2_pair_kernel<1, false, false>), SDF_K(extz2_pair_kernel<1, true, false>),
      SDF_K(extz2_pair_kernel<2, false, false>), SDF_K(extz2_pair_kernel<2, true, false>),
      SDF_K(extz2_pair_kernel<3, false, false>), SDF_K(extz2_pair_kernel<3, true, false>),
      SDF_K(extz2_pair_kernel<4, false, false>), SDF_K(extz2_pair_kernel<4, true, false>),
      SDF_K(extz2_pair_kernel<6, false, false>), SDF_K(extz2_pair_kernel<6, true, false>),
      SDF_K(extz2_pair_kernel<8, false, false>), SDF_K(extz2_pair_kernel<8, true, false>),
      SDF_K(extz2_pair_kernel<3, true, true>), SDF_K(extz2_pair_kernel<6, true, true>),
      SDF_K(extz2_pair_mixed_kernel<2>), SDF_K(extz2_pair_mixed_kernel<3>), SDF_K(extz2_pair_mixed_kernel<4>),
      SDF_K(extz2_pair_mixed_kernel<5>), SDF_K(extz2_pair_mixed_kernel<6>), SDF_K(extz2_pair_mixed_kernel<8>),
      SDF_K(extz2_pair_mixed_kernel<9>),
      SDF_K(extz2_stripe_kernel<1>), SDF_K(extz2_stripe_kernel<2>), SDF_K(extz2_stripe_kernel<4>),
      SDF_K(extz2_bstripe_kernel<1>), SDF_K(extz2_bstripe_kernel<2>), SDF_K(extz2_bstripe_kernel<4>),
      SDF_K(extz2_strip_kernel), SDF_K(extz2_lane_kernel)};
#undef SDF_K
  bool general_ok = true;
  for (size_t i = 0; i < sizeof(dyn_lds_kernels) / sizeof(dyn_lds_kernels[0]); ++i) {
    const bool ok = hipFuncSetAttribute(dyn_lds_kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, want_lds) == hipSuccess;
    if (i < 5) general_ok = general_ok && ok;
  }
  if (general_ok) ctx->max_dyn_lds = want_lds;
  (void)hipGetLastError();
  // (per context, hence per device: a process-wide once-flag would leave a second GPU's copy of the kernel at 64 KiB)
  // (refused: the kernel keeps the 64 KiB every kernel has, and sdf_chain_batch's largest LDS class ends there)
  const int chain_lds = std::max(ctx->max_dyn_lds, 65536);
  const bool chain_lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&sdf::chain_wave_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, chain_lds) == hipSuccess;
  ctx->chain_classes[7] = chain_lds_ok ? chain_lds : 65536;
  (void)hipGetLastError();
  lap.at("attributes");
  if (!pipeline_streams) {
    ctx->pipeline_ok = false;
  } else if (hipStreamCreateWithFlags(&ctx->dp_stream[0], hipStreamNonBlocking) != hipSuccess ||
             hipStreamCreateWithFlags(&ctx->dp_stream[1], hipStreamNonBlocking) != hipSuccess ||
             hipStreamCreateWithFlags(&ctx->tb_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    ctx->pipeline_ok = false;
  }
  // (three streams of our own: the runtime multiplexes streams onto GPU_MAX_HW_QUEUES -- default 4 -- hardware
  // queues, and two of ours landing on one queue serialises what the pipeline wants side by side; with the
  // caller's stream that makes four)
  g_live_contexts.fetch_add(1);
  if (cfg.debug_timing) fprintf(stderr, "[sdf_create device %d: %.1f ms]\n", device, ms_since(lap.t0));
  return ctx;
}

void mark_internal_context(sdf_ctx *c) {
  if (!c || c->is_part) return;
  c->is_part = true;
  g_live_contexts.fetch_sub(1);
}

// ---- one resident pool read by several contexts of a device (include/sedef_hip.h: sdf_pool_share) ----
static std::mutex g_share_mu;  // every context's view_of / views

// (g_share_mu held) the view gives its owner's pool back: an empty pool of its own
static void drop_view_locked(sdf_ctx *v) {
  if (sdf_ctx *owner = v->view_of) {
    auto &l = owner->views;
    l.erase(std::remove(l.begin(), l.end(), v), l.end());
    v->view_of = nullptr;
  }
  v->an_pool.drop_borrow();
  v->pool_bytes = 0;
  v->pool_epoch += 1;
}

int pool_writable(sdf_ctx *ctx, bool keep_view) {
  std::lock_guard<std::mutex> g(g_share_mu);
  if (!ctx->views.empty()) {
    ctx->err = "pool is shared: other contexts hold views of it (sdf_pool_share)";
    return SDF_ERR_INVALID;
  }
  if (ctx->an_pool.borrowed) {
    if (keep_view) {
      ctx->err = "pool is shared: this context holds a view of another context's pool and cannot add to it";
      return SDF_ERR_INVALID;
    }
    drop_view_locked(ctx);
  }
  return SDF_OK;
}

extern "C" int sdf_pool_share(sdf_ctx *dst, const sdf_ctx *src_c) {
  sdf_ctx *src = const_cast<sdf_ctx *>(src_c);  // (the owner's list of views and a marker on its stream)
  if (!dst) return SDF_ERR_INVALID;
  sdf_ctx *ctx = dst;
  ctx->err.clear();
  std::lock_guard<std::mutex> g(g_share_mu);
  auto invalid = [&](const char *why) {
    ctx->err = std::string("sdf_pool_share: ") + why;
    return SDF_ERR_INVALID;
  };
  if (!src || src == dst) return invalid("the source is the destination, or none");
  if (src->device != dst->device) return invalid("the two contexts are on different devices");
  if (src->an_pool.borrowed) return invalid("the source is itself a view");
  if (!dst->views.empty()) return invalid("pool is shared: other contexts hold views of the destination's pool");
  SDF_HIP(hipSetDevice(dst->device));
  // dst's streams see what the owner has enqueued so far: its uploads
  hipEvent_t ev = nullptr;
  SDF_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, src->stream);
  for_each_stream(dst, [&](hipStream_t q) {
    if (q && e == hipSuccess) e = hipStreamWaitEvent(q, ev, 0);
  });
  (void)hipEventDestroy(ev);  // (released once it has completed)
  SDF_HIP(e);
  drop_view_locked(dst);  // (a view of another owner, if it held one)
  dst->an_pool.borrow(src->an_pool.p, src->an_pool.cap);
  dst->pool_bytes = src->pool_bytes;
  dst->pool_epoch += 1;
  dst->view_of = src;
  src->views.push_back(dst);
  return SDF_OK;
}

extern "C" void sdf_destroy(sdf_ctx *ctx) {
  if (!ctx) return;
  if (!ctx->is_part) g_live_contexts.fetch_sub(1);
  (void)hipSetDevice(ctx->device);
  while (!ctx->lanes.empty()) close_lanes(ctx, ctx->lanes.back());  // (lanes still open go first: they are views of this pool)
  for_each_stream(ctx, [](hipStream_t q) { if (q) (void)hipStreamSynchronize(q); });
  {  // a view leaves its owner's list; an owner's views (the caller's error: the owner outlives its views) are left with an
     // empty pool, so that their later calls answer SDF_ERR_INVALID instead of reading freed memory
    std::lock_guard<std::mutex> g(g_share_mu);
    drop_view_locked(ctx);
    while (!ctx->views.empty()) drop_view_locked(ctx->views.back());
  }
  for (auto ev : ctx->events) (void)hipEventDestroy(ev);
  for (sdf_search_index *h : ctx->indexes) {  // (the handles still live go with their context: include/sedef_hip.h)
    h->d_loc.release(), h->d_sorted.release();
    delete h;
  }
  ctx->indexes.clear();
  for_each_device_buffer(ctx, [](DevBuf &b) { b.release(); });
  for_each_host_buffer(ctx, [](HostBuf &b) { b.release(); });
  if (ctx->rerun_ctx) sdf_destroy(ctx->rerun_ctx);
  if (ctx->part_ctx) sdf_destroy(ctx->part_ctx);
  if (ctx->part_ev) (void)hipEventDestroy(ctx->part_ev);
  for_each_stream(ctx, [](hipStream_t q) { if (q) (void)hipStreamDestroy(q); });
  if (!ctx->pool_shared) delete ctx->pool;
  delete ctx->cut;
  delete ctx;
}

extern "C" float sdf_last_ms(const sdf_ctx *ctx, int which) {
  if (!ctx || which < 0 || which > 6) return 0.f;
  return ctx->ms[which];
}

extern "C" int sdf_last_launches(const sdf_ctx *ctx) { return ctx ? ctx->launches : 0; }
extern "C" long long sdf_last_paired(const sdf_ctx *ctx) { return ctx ? ctx->paired : 0; }
extern "C" long long sdf_last_reran(const sdf_ctx *ctx) { return ctx ? ctx->reran : 0; }
extern "C" long long sdf_last_lane_tasks(const sdf_ctx *ctx) { return ctx ? ctx->lane_tasks : 0; }
extern "C" int sdf_last_chain_classes(const sdf_ctx *ctx, int64_t out[8]) {
  if (!ctx || !out) return SDF_ERR_INVALID;
  std::copy(ctx->chain_classes, ctx->chain_classes + 8, out);
  return SDF_OK;
}
extern "C" int sdf_last_traceback_classes(const sdf_ctx *ctx, int64_t out[14]) {
  if (!ctx || !out) return SDF_ERR_INVALID;
  std::copy(ctx->tb_classes, ctx->tb_classes + 14, out);
  return SDF_OK;
}

// Buffers sized once (include/sedef_hip.h).  The bounds per task are the planner's: a launch-order entry per task and
// stripe / block of columns, a CIGAR staging slot of qlen + tlen + 2 words.
extern "C" int sdf_reserve(sdf_ctx *ctx, size_t max_tasks, size_t max_bases, size_t workspace_bytes, uint32_t flags) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  SDF_HIP(hipSetDevice(ctx->device));
  Lap lap{ctx->cfg.debug_timing != 0, "[sdf_reserve: %s %.1f ms]\n", 20};  // (the sections that took more than 20 ms)
  const size_t n = std::max<size_t>(max_tasks, 1);
  const size_t words = max_bases / 16 + max_bases / 32 + 4 * n + 16;  // (packed sequences: two roundings per sequence)
  const size_t cig_words = max_bases + 2 * n + 16;
  const size_t nord = 3 * n + max_bases / 16 + 1024;
  // pinned staging (registered huge pages unless sdf_config.pin_register says otherwise: sdf_ctx.h, HostBuf::reserve_huge)
  const bool reg_small = ctx->cfg.pin_register >= 1, reg_big = ctx->cfg.pin_register >= 2;
  SDF_HIP(ctx->host_pool.reserve_pinned(reg_small, std::max(words * 4, n * sizeof(sdf::PackRec))));  // (packed sequences, or a record per task of sdf_extz2_batch_pairs)
  SDF_HIP(ctx->pk_recs.reserve_exact(n * sizeof(sdf::PackRec)));
  SDF_HIP(ctx->host_plan.reserve_pinned(reg_small, n * sizeof(PlanTask)));
  SDF_HIP(ctx->host_order.reserve_pinned(reg_small, nord * sizeof(int32_t)));
  SDF_HIP(ctx->host_lane.reserve_pinned(reg_small, n * sizeof(LaneRec)));
  // (results + CIGAR words: a quarter of the CIGAR bound -- the stage's rounds fill a tenth of it)
  SDF_HIP(ctx->host_out.reserve_pinned(reg_small, n * ((flags & SDF_RESERVE_BRIEF) ? sizeof(sdf_result_brief) : sizeof(sdf_result)) +
                                      cig_words / 4 * 4 + 64));
  if (ctx->host_tasks.size() < n) ctx->host_tasks.resize(n);
  lap("pinned staging");
  // device
  SDF_HIP(ctx->h_pool.reserve_exact(words * 4));
  SDF_HIP(ctx->h_out.reserve_exact(n * sizeof(sdf_result)));
  SDF_HIP(ctx->h_brief.reserve_exact(n * sizeof(sdf_result_brief)));
  SDF_HIP(ctx->h_cig.reserve_exact(cig_words * 4));
  SDF_HIP(ctx->stage_ws.reserve_exact(cig_words * 4));
  SDF_HIP(ctx->plan_buf.reserve_exact(2 * n * sizeof(PlanTask)));  // (host-planned records, the lane tasks' behind them)
  SDF_HIP(ctx->order_buf.reserve_exact(nord * sizeof(int32_t)));
  SDF_HIP(ctx->misc_buf.reserve_exact(SDF_MISC_PARTS * 8 + ((n + 1023) / 1024 + 1) * 8));
  SDF_HIP(ctx->claim_buf.reserve_exact(kClaimSets * 8 * sizeof(unsigned)));
  SDF_HIP(ctx->ln_recs.reserve_exact(n * sizeof(LaneRec)));
  SDF_HIP(ctx->ln_keys.reserve_exact(n * 8));
  SDF_HIP(ctx->ln_vals.reserve_exact(n * 8));
  SDF_HIP(ctx->ln_sizes.reserve_exact(n * 32 + 64));
  SDF_HIP(ctx->ln_bins.reserve_exact((size_t)kLaneBins * (4 + 4 + 4 + 8 + 8) + (size_t)(kLaneBins / kLaneScanBlock) * 24 + 256));
  lap("device buffers");
  {  // (the library sort / scan of the lane tasks' planning: sdf_launch.hip, launch_lane)
    size_t t_sort = 0, t_scan = 0;
    SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                               (uint32_t *)nullptr, (int)n, 0, 20, ctx->stream));
    SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n,
                                             ctx->stream));
    SDF_HIP(ctx->ln_tmp.reserve_exact(std::max(t_sort, t_scan) + 256));
  }
  // the streams the pipeline would create the first time it wants them (a stream is a hardware queue: 7-15 ms each to set
  // up -- the stage's first two rounds spent 35 ms on five of them)
  lap("sort / scan scratch");
  if (flags & SDF_RESERVE_FEW_STREAMS) ctx->aux_limit = 0;
  if (ctx->pipeline_ok) {
    if (!ctx->lane_stream && create_lane_stream(ctx, &ctx->lane_stream) != hipSuccess) ctx->lane_stream = nullptr;
    for (size_t a = 0; a < 4 && a < ctx->aux_limit; ++a)
      if (!ctx->aux_stream[a] && hipStreamCreateWithFlags(&ctx->aux_stream[a], hipStreamNonBlocking) != hipSuccess) ctx->aux_stream[a] = nullptr;
    (void)hipGetLastError();
  }
  lap("pipeline streams");
  if (workspace_bytes) {
    const size_t ws = std::min(workspace_bytes, ctx->ws_budget);
    if (ctx->dir_ws.reserve_exact(ws) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "cannot allocate the direction-matrix workspace";
      return SDF_ERR_NOMEM;
    }
  }
  lap("direction-flag workspace");
  if (flags & SDF_RESERVE_ANCHORS) SDF_HIP(ctx->host_an.reserve_pinned(reg_big, (size_t)48 << 20));
  lap("pinned anchors staging");
  if (flags & SDF_RESERVE_ANCHORS) {  // two copies of a short sequence: a handful of anchors through every kernel of the path
    char seq[192];
    uint32_t x = 12345u;
    for (int i = 0; i < 96; ++i) {
      x = x * 1664525u + 1013904223u;
      seq[i] = seq[96 + i] = "ACGT"[x >> 30];
    }
    sdf_anchor_pair pr;
    memset(&pr, 0, sizeof(pr));
    pr.q_off = 0;
    pr.r_off = 96;
    pr.qlen = pr.rlen = 96;
    sdf_anchor out[256];
    int64_t off[2];
    size_t used = 0;
    (void)sdf_anchors_batch(ctx, &pr, 1, seq, sizeof(seq), 11, out, 256, off, &used);
    ctx->err.clear();
  }
  lap("anchors warm-up call");
  {  // the stream's first asynchronous copy in each direction costs its caller ~8 ms (the runtime sets its copy path up): here,
     // not in front of a super-batch's upload and its anchors' way back (profiles/r06_stage_timeline.txt)
    const size_t probe = std::min<size_t>({(size_t)1 << 20, ctx->host_pool.cap, ctx->h_pool.cap, ctx->host_out.cap, ctx->h_out.cap});
    if (probe) {
      SDF_HIP(hipMemcpyAsync(ctx->h_pool.p, ctx->host_pool.p, probe, hipMemcpyHostToDevice, ctx->stream));
      // (device to host: a copy of the size the rounds' results have -- a small one does not take the path a 17 MB one takes)
      const size_t back = std::min<size_t>({(size_t)32 << 20, ctx->host_out.cap, ctx->h_out.cap});
      SDF_HIP(hipMemcpyAsync(ctx->host_out.p, ctx->h_out.p, back, hipMemcpyDeviceToHost, ctx->stream));
      SDF_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  lap("first asynchronous copies");
  return SDF_OK;
}

extern "C" size_t sdf_device_bytes(const sdf_ctx *ctx) {
  if (!ctx) return 0;
  size_t sum = 0;
  for_each_device_buffer(ctx, [&](const DevBuf &b) { sum += b.held_bytes(); });
  for (const sdf_search_index *h : ctx->indexes) sum += h->d_loc.held_bytes() + h->d_sorted.held_bytes();
  if (ctx->part_ctx) sum += sdf_device_bytes(ctx->part_ctx);
  if (ctx->rerun_ctx) sum += sdf_device_bytes(ctx->rerun_ctx);
  for (const sdf_search_lanes *l : ctx->lanes)
    for (const sdf_ctx *lane : l->lane) sum += sdf_device_bytes(lane);
  return sum;
}

extern "C" size_t sdf_debug_live_device_bytes(void) { return (size_t)DevBuf::live_bytes.load(); }
