// The C ABI: several pairs of the search driver in flight on one GPU (include/sedef_hip.h: sdf_search_lanes_open / _close,
// sdf_search_pairs_indexed).  A lane is a child context of the owner: a view of the owner's pool (sdf_pool_share), a stream and
// per-call buffers of its own; the handles stay the owner's and are only read.  The rounds of one pair are those of
// sdf_search_pair_indexed_wide (sdf_driver_api.hip: pair_handles_run); the queue the lanes' threads take the pairs from:
// sdf_job_queue.h.  No kernel is launched from here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "sdf_entry.h"
#include "sdf_job_queue.h"

using namespace sdf;

namespace {
// a lanes object this context holds (looked up by address, as handles are)
bool lanes_live(const sdf_ctx *ctx, const sdf_search_lanes *l) {
  return l && std::find(ctx->lanes.begin(), ctx->lanes.end(), l) != ctx->lanes.end();
}
}  // namespace

void close_lanes(sdf_ctx *owner, sdf_search_lanes *lanes) {
  for (sdf_ctx *lane : lanes->lane) sdf_destroy(lane);  // (waits for the lane's stream and drops its view)
  auto &l = owner->lanes;
  l.erase(std::remove(l.begin(), l.end(), lanes), l.end());
  delete lanes;
}

extern "C" int sdf_search_lanes_open(sdf_ctx *ctx, int n_lanes, sdf_search_lanes **out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!out) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_lanes_open: invalid arguments");
  *out = nullptr;
  if (n_lanes < 1 || n_lanes > SDF_SEARCH_LANES_MAX) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_lanes_open: n_lanes outside 1 .. 16");
  SDF_HIP(hipSetDevice(ctx->device));
  sdf_search_lanes *L = new sdf_search_lanes();
  L->owner = ctx;
  auto fail = [&](int rc, std::string why) {
    for (sdf_ctx *lane : L->lane) sdf_destroy(lane);
    delete L;
    return refuse(ctx, rc, std::move(why));
  };
  // (with the owner's settings, not the environment's, as every context the library makes for itself)
  sdf_config cfg = ctx->cfg;
  cfg.workspace_gib = 0;
  cfg.debug_plan = 0;
  for (int i = 0; i < n_lanes; i++) {
    sdf_ctx *lane = create_context(ctx->device, ctx->ws_budget, &cfg, false);
    if (!lane) return fail(SDF_ERR_NOMEM, "sdf_search_lanes_open: cannot create lane " + std::to_string(i) + ": " + sdf_last_error(nullptr));
    mark_internal_context(lane);  // (not another user of the process's CPUs)
    lane->ws_budget = ctx->ws_budget;  // (what decides whether a round's long growths run on the device is the owner's)
    L->lane.push_back(lane);
    if (int rc = sdf_pool_share(lane, ctx)) return fail(rc, "sdf_search_lanes_open: lane " + std::to_string(i) + ": " + lane->err);
    // the buffers of a round whose size no pair changes; everything else is reserved by need
    hipError_t e = lane->dr_status.reserve(sizeof(sdf_search_accept_status) + 16);
    if (e == hipSuccess) e = lane->dr_limit.reserve(16);
    if (e == hipSuccess) e = lane->fo_need.reserve(8);
    if (e == hipSuccess) e = lane->ac_go.reserve(4);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(e == hipErrorOutOfMemory ? SDF_ERR_NOMEM : SDF_ERR_HIP, std::string("sdf_search_lanes_open: ") + hipGetErrorString(e));
    }
  }
  ctx->lanes.push_back(L);
  *out = L;
  return SDF_OK;
}

extern "C" int sdf_search_lanes_close(sdf_ctx *ctx, sdf_search_lanes *lanes) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!lanes) return SDF_OK;
  if (!lanes_live(ctx, lanes)) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_lanes_close: not live lanes of this context");
  SDF_HIP(hipSetDevice(ctx->device));
  close_lanes(ctx, lanes);
  return SDF_OK;
}

extern "C" int sdf_search_pairs_indexed(sdf_ctx *ctx, sdf_search_lanes *lanes, const sdf_search_pair_job *jobs, size_t n_jobs,
                                        const sdf_search_pair_params *params, size_t n_wide_max, sdf_search_pair_hit *out, size_t cap,
                                        size_t *used, uint64_t *first, sdf_search_pair_stats *stats) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!lanes || !params || !used || !first || (cap && !out) || (n_jobs && (!jobs || !stats)))
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_pairs_indexed: invalid arguments");
  if (!lanes_live(ctx, lanes)) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_pairs_indexed: not live lanes of this context");
  try {  // (no exception crosses the ABI: the call's own vectors may not be had)
  // every job's parameters; the checks of all jobs before the first launch: the handles first, then the ranges
  std::vector<sdf_search_pair_params> P(n_jobs, *params);
  for (size_t j = 0; j < n_jobs; j++) P[j].same_genome = P[j].extend.same_genome = jobs[j].same_genome != 0;
  const char *why = nullptr;
  for (size_t j = 0; j < n_jobs; j++)
    if (int rc = pair_handles_valid(ctx, jobs[j].q, jobs[j].r, &P[j], &why)) return refuse(ctx, rc, "job " + std::to_string(j) + ": " + why);
  for (size_t j = 0; j < n_jobs; j++)
    if (int rc = pair_handles_ranges(sdf_pool_bytes(ctx), jobs[j].q, jobs[j].r, &P[j], n_wide_max, &why))
      return refuse(ctx, rc, "job " + std::to_string(j) + ": " + why);
  first[0] = 0;
  *used = 0;
  if (n_jobs == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  SDF_HIP(hipStreamSynchronize(ctx->stream));  // (what the owner enqueued before this call is there for every lane)
  std::vector<uint64_t> size(n_jobs);
  for (size_t j = 0; j < n_jobs; j++) size[j] = jobs[j].q->loc.size();
  std::vector<std::vector<sdf_search_pair_hit>> hits(n_jobs);
  std::vector<std::string> text(n_jobs);
  std::vector<int> before;
  for (const sdf_ctx *lane : lanes->lane) before.push_back(lane->launches);
  // a lane's thread: the job on the lane's stream and in the lane's buffers; the handles are read, never written
  const std::vector<int> code = run_job_queue(lanes->lane.size(), largest_first(size), [&](size_t t, size_t j) {
    sdf_ctx *lane = lanes->lane[t];
    if (hipSetDevice(lane->device) != hipSuccess) {
      text[j] = "hipSetDevice failed";
      return (int)SDF_ERR_HIP;
    }
    try {
      const int rc = pair_handles_run(lane, ctx, jobs[j].q, jobs[j].r, &P[j], n_wide_max, hits[j], &stats[j]);
      if (rc != SDF_OK) text[j] = lane->err;
      return rc;
    } catch (const std::bad_alloc &) {  // (the host lists of a pair: nothing leaves a lane's thread)
      return (int)SDF_ERR_NOMEM;
    }
  });
  for (size_t t = 0; t < lanes->lane.size(); t++) ctx->launches += lanes->lane[t]->launches - before[t];
  // a job that failed in flight: the lowest index; the jobs behind it in the queue were not started
  for (size_t j = 0; j < n_jobs; j++)
    if (code[j] != SDF_OK && code[j] != kJobNotStarted) {
      if (code[j] == SDF_ERR_NOMEM && text[j].empty()) text[j] = "out of host memory";
      if (code[j] == kJobThrew) return refuse(ctx, SDF_ERR_HIP, "job " + std::to_string(j) + ": the lane's thread left the job by an exception");
      return refuse(ctx, code[j], "job " + std::to_string(j) + ": " + text[j]);
    }
  for (size_t j = 0; j < n_jobs; j++) first[j + 1] = first[j] + hits[j].size();
  *used = (size_t)first[n_jobs];
  if (*used > cap)
    return refuse(ctx, SDF_ERR_CIGAR_OVERFLOW, "the " + std::to_string(n_jobs) + " pairs have " + std::to_string(*used) + " hits, more than cap");
  for (size_t j = 0; j < n_jobs; j++)
    if (!hits[j].empty()) memcpy(out + first[j], hits[j].data(), hits[j].size() * sizeof(sdf_search_pair_hit));
  return SDF_OK;
  } catch (const std::bad_alloc &) {
    *used = 0;
    return refuse(ctx, SDF_ERR_NOMEM, "sdf_search_pairs_indexed: out of host memory");
  }
}
