// The C ABI: the device and uploading forms of the search filter -- uppercase and q-gram verdicts per pair of pool ranges
// (search_filter.hip; include/sedef_hip.h states the contract) -- and of the tasks of the rolled intervals and of the hits,
// with their launches.  The `_host` forms and the checks: search_host.hip.
#include <hip/hip_runtime.h>

#include "sdf_entry.h"
#include "search_host.h"

using namespace sdf;

namespace {
// the launches: the wavefront class over all n tasks (hist_only: its histogram pass alone) and -- with_long -- the long class,
// each in pieces of FILTER_LAUNCH_TASKS tasks
int filter_launch(sdf_ctx *ctx, const sdf_filter_params &P, const sdf_filter_task *d_tasks, size_t n, bool rev, bool with_long,
                  sdf_filter_rec *d_out, hipStream_t st, bool hist_only = false) {
  const char *pool = (const char *)ctx->an_pool.p;
  const long long pool_bytes = (long long)ctx->pool_bytes;
  using Kernel = void (*)(const sdf_filter_task *, int, const char *, long long, sdf_filter_params, sdf_filter_rec *);
  const Kernel wave = hist_only ? (rev ? search_filter_kernel<1, true, false> : search_filter_kernel<1, false, false>)
                                : (rev ? search_filter_kernel<1, true, true> : search_filter_kernel<1, false, true>);
  const Kernel wide = rev ? search_filter_kernel<FILTER_LONG_WAVES, true, true> : search_filter_kernel<FILTER_LONG_WAVES, false, true>;
  for (size_t at = 0; at < n; at += FILTER_LAUNCH_TASKS) {
    const size_t m = std::min(FILTER_LAUNCH_TASKS, n - at);
    hipLaunchKernelGGL(wave, dim3((unsigned)m), dim3(64), 0, st, d_tasks + at, (int)m, pool, pool_bytes, P, d_out + at);
    if (with_long) hipLaunchKernelGGL(wide, dim3((unsigned)m), dim3(64 * FILTER_LONG_WAVES), 0, st, d_tasks + at, (int)m, pool, pool_bytes, P, d_out + at);
    SDF_HIP(hipGetLastError());
    ctx->launches += with_long ? 2 : 1;
  }
  return SDF_OK;
}
}  // namespace

static int filter_device(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *d_tasks, size_t n, int any_rc, bool with_long,
                         bool hist_only, sdf_filter_rec *d_out, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) return SDF_OK;
  if (!d_tasks || !d_out) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_filter_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = filter_scalars(params, n, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (int rc = filter_launch(ctx, *params, d_tasks, n, any_rc != 0, with_long, d_out, st, hist_only)) return rc;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_search_filter_device(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *d_tasks, size_t n, int any_rc,
                                        sdf_filter_rec *d_out, void *stream) {
  return filter_device(ctx, params, d_tasks, n, any_rc, true, false, d_out, stream);
}

// For profiles/search_filter.py, not in the header: the device form's wavefront-class launch alone (the tasks of the long class get
// no record) -- phase 1 --, or that launch with workgroups that leave behind the histogram pass -- phase 0: d_out's records are
// then NOT the pairs'.  The first against the device form is the cost of the long class's launch over tasks that are not its own,
// the second against the first the share of the histogram pass.
extern "C" int sdf_search_filter_phase_device(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *d_tasks, size_t n,
                                              int any_rc, int phase, sdf_filter_rec *d_out, void *stream) {
  return filter_device(ctx, params, d_tasks, n, any_rc, false, phase == 0, d_out, stream);
}

extern "C" int sdf_search_filter(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *tasks, size_t n, sdf_filter_rec *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) return SDF_OK;
  if (!tasks || !out) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_filter: invalid arguments");
  const char *why = nullptr;
  if (int rc = filter_scalars(params, n, &why)) return refuse(ctx, rc, why);
  bool any_rc = false, any_long = false;
  std::string text;
  if (int rc = filter_tasks(tasks, n, ctx->pool_bytes, &any_rc, &any_long, &text)) return refuse(ctx, rc, text);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the pool's uploads were enqueued there)
  if (int rc = upload_all(ctx, st, {{ctx->sf_tasks, tasks, n * sizeof(sdf_filter_task)}})) return rc;
  SDF_HIP(ctx->sf_out.reserve(n * sizeof(sdf_filter_rec)));
  if (int rc = filter_launch(ctx, *params, (const sdf_filter_task *)ctx->sf_tasks.p, n, any_rc, any_long, (sdf_filter_rec *)ctx->sf_out.p, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->sf_out.p, n * sizeof(sdf_filter_rec), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_search_filter_tasks_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                              const uint64_t *d_first, const sdf_search_interval *d_intervals,
                                              const sdf_search_roll_rec *d_rolls, size_t n_max, int64_t len_q, int64_t len_r,
                                              int32_t init_len, int64_t q_off, int q_rc, int64_t r_off, int r_rc, int allow_extend,
                                              sdf_filter_task *d_out, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0 || n_max == 0) return SDF_OK;
  if (!d_q || !d_windows || !d_first || !d_intervals || !d_rolls || !d_out)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_filter_tasks_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = filter_tasks_scalars(nq, n_max, len_q, len_r, init_len, q_off, r_off, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const FilterTaskArgs A{len_q, len_r, q_off, r_off, init_len, q_rc != 0, r_rc != 0, allow_extend != 0};
  hipLaunchKernelGGL(search_filter_tasks_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, st, d_q, (int)nq, d_windows, d_first,
                     d_intervals, d_rolls, (int)n_max, A, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// ---- the tasks of the hits (the reference's second filter(), src/search.cc:356) ----

extern "C" int sdf_search_hit_tasks_device(sdf_ctx *ctx, const sdf_search_hit *d_hits, size_t n, const uint64_t *d_count, int64_t len_q,
                                           int64_t len_r, int64_t q_off, int q_rc, int64_t r_off, int r_rc, sdf_filter_task *d_out,
                                           void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) return SDF_OK;
  const char *why = nullptr;
  if (int rc = hit_tasks_scalars(n, len_q, len_r, q_off, r_off, &why)) return refuse(ctx, rc, why);
  if (!d_hits || !d_out) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_hit_tasks_device: invalid arguments");
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const FilterTaskArgs A{len_q, len_r, q_off, r_off, 0, q_rc != 0, r_rc != 0, 0};
  hipLaunchKernelGGL(search_hit_tasks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_hits, (int)n, d_count, A, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}
