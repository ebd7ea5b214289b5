// The C ABI: the search filter -- uppercase and q-gram verdicts per pair of pool ranges (search_filter.hip; include/sedef_hip.h
// states the contract) -- and the tasks of the rolled intervals.  sdf_search_filter_host and sdf_search_filter_tasks_host are
// those in plain C++; the verdict, minqg and the task of an interval are the functions of sdf_kernels.h the kernels use.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sdf_entry.h"

using namespace sdf;

namespace {
// what every form checks of its parameters and n
int filter_scalars(const sdf_filter_params *P, size_t n, const char **why) {
  if (!P) return *why = "search filter: invalid arguments", SDF_ERR_INVALID;
  if (!std::isfinite(P->max_error) || !std::isfinite(P->max_edit_error) || !std::isfinite(P->gap_frequency))
    return *why = "search filter: a parameter that is not finite", SDF_ERR_INVALID;
  if (P->reserved != 0) return *why = "search filter: reserved != 0 in the parameters", SDF_ERR_UNSUPPORTED;
  if (n > 0x7fffffffu) return *why = "search filter: more than 2^31 - 1 tasks in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the host forms of their tasks, in order; the first refusal is the call's
int filter_tasks(const sdf_filter_task *tasks, size_t n, size_t pool_bytes, bool *any_rc, bool *any_long, std::string *why) {
  *any_rc = *any_long = false;
  for (size_t i = 0; i < n; i++) {
    const sdf_filter_task &T = tasks[i];
    if ((T.flags & ~(uint32_t)(SDF_FILTER_Q_RC | SDF_FILTER_R_RC | SDF_FILTER_SKIP)) || T.reserved != 0)
      return *why = "search filter: task " + std::to_string(i) + ": unknown flag or reserved != 0", SDF_ERR_UNSUPPORTED;
    if (!in_range(T.q_off, (int64_t)T.q_len, pool_bytes) || !in_range(T.r_off, (int64_t)T.r_len, pool_bytes))
      return *why = "search filter: task " + std::to_string(i) + ": range outside the resident pool", SDF_ERR_INVALID;
    if (T.flags & SDF_FILTER_SKIP) continue;
    *any_rc |= (T.flags & (SDF_FILTER_Q_RC | SDF_FILTER_R_RC)) != 0;
    *any_long |= T.q_len > FILTER_WAVE_MAX_LEN || T.r_len > FILTER_WAVE_MAX_LEN;
  }
  return SDF_OK;
}

// rev_dna (reference: src/common.h:72-87,93) of a character below 128
inline unsigned char filter_rev_dna(unsigned char c) {
  switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'a': return 't';
    case 'c': return 'g';
    case 'g': return 'c';
    case 't': return 'a';
    default: return 'N';
  }
}
// one side as the header states it: up, and its grams counted into hist
int32_t filter_side_host(const char *s, int32_t len, bool rc, std::vector<uint32_t> &hist) {
  int32_t up = 0;
  uint32_t g = 0;
  for (int32_t i = 0; i < len; i++) {
    unsigned char c = (unsigned char)(rc ? s[len - 1 - i] : s[i]) & 127;
    if (rc) c = filter_rev_dna(c);
    up += c >= 'A' && c <= 'Z';
    const unsigned char u = c & 0xDF;
    g = ((g << 2) | (u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u)) & (FILTER_GRAMS - 1);
    if (i >= 4) hist[g]++;
  }
  return up;
}

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

// what every form of the task builder checks of its scalars (n: the intervals, or the lanes of the device form)
int filter_tasks_scalars(size_t nq, size_t n, int64_t len_q, int64_t len_r, int32_t init_len, int64_t q_off, int64_t r_off, const char **why) {
  if (init_len < 1) return *why = "search filter tasks: init_len < 1", SDF_ERR_INVALID;
  if (len_q < 0 || len_r < 0 || q_off < 0 || r_off < 0) return *why = "search filter tasks: a negative length or offset", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search filter tasks implement init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x7fffffffu || n > 0x7fffffffu || len_q > 0x7fffffff || len_r > 0x7fffffff)
    return *why = "search filter tasks: more than 2^31 - 1 query minimizers, intervals or bases in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_filter_host(const char *pool, size_t pool_bytes, const sdf_filter_params *params, const sdf_filter_task *tasks,
                                      size_t n, sdf_filter_rec *out) {
  if (n == 0) return SDF_OK;
  if (!tasks || !out || (pool_bytes && !pool)) return SDF_ERR_INVALID;
  const char *why = nullptr;
  if (int rc = filter_scalars(params, n, &why)) return rc;
  bool any_rc = false, any_long = false;
  std::string text;
  if (int rc = filter_tasks(tasks, n, pool_bytes, &any_rc, &any_long, &text)) return rc;
  std::vector<uint32_t> hq(FILTER_GRAMS), hr(FILTER_GRAMS);
  for (size_t i = 0; i < n; i++) {
    const sdf_filter_task &T = tasks[i];
    if (T.flags & SDF_FILTER_SKIP) {
      out[i] = sdf_filter_rec{0, 0, 0, 0, SDF_FILTER_SKIPPED};
      continue;
    }
    std::fill(hq.begin(), hq.end(), 0u);
    std::fill(hr.begin(), hr.end(), 0u);
    const int32_t q_up = filter_side_host(pool + T.q_off, T.q_len, (T.flags & SDF_FILTER_Q_RC) != 0, hq);
    const int32_t r_up = filter_side_host(pool + T.r_off, T.r_len, (T.flags & SDF_FILTER_R_RC) != 0, hr);
    int64_t dist = 0;
    for (int b = 0; b < FILTER_GRAMS; b++) dist += std::min(hq[b], hr[b]);
    out[i] = filter_verdict(q_up, r_up, (int32_t)dist, std::max(T.q_len, T.r_len), *params);
  }
  return SDF_OK;
}

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
  SDF_HIP(ctx->sf_tasks.reserve(n * sizeof(sdf_filter_task)));
  SDF_HIP(ctx->sf_out.reserve(n * sizeof(sdf_filter_rec)));
  SDF_HIP(hipMemcpyAsync(ctx->sf_tasks.p, tasks, n * sizeof(sdf_filter_task), hipMemcpyHostToDevice, st));
  if (int rc = filter_launch(ctx, *params, (const sdf_filter_task *)ctx->sf_tasks.p, n, any_rc, any_long, (sdf_filter_rec *)ctx->sf_out.p, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->sf_out.p, n * sizeof(sdf_filter_rec), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_search_filter_tasks_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                            const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, int64_t len_q,
                                            int64_t len_r, int32_t init_len, int64_t q_off, int q_rc, int64_t r_off, int r_rc,
                                            int allow_extend, sdf_filter_task *out) {
  if (nq == 0) return SDF_OK;
  if (!q || !windows || !first || first[0] != 0) return SDF_ERR_INVALID;
  for (size_t i = 0; i < nq; i++)
    if (first[i + 1] < first[i]) return SDF_ERR_INVALID;
  const uint64_t n = first[nq];
  const char *why = nullptr;
  if (int rc = filter_tasks_scalars(nq, n > 0x7fffffffu ? (size_t)0x80000000u : (size_t)n, len_q, len_r, init_len, q_off, r_off, &why)) return rc;
  if (n && (!intervals || !rolls || !out)) return SDF_ERR_INVALID;
  const FilterTaskArgs A{len_q, len_r, q_off, r_off, init_len, q_rc != 0, r_rc != 0, allow_extend != 0};
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++) out[t] = filter_task_of(A, q[i].loc, windows[i], intervals[t], rolls[t]);
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

namespace {
// what both forms of the hits' task builder check of their scalars
int hit_tasks_scalars(size_t n, int64_t len_q, int64_t len_r, int64_t q_off, int64_t r_off, const char **why) {
  if (len_q < 0 || len_r < 0 || q_off < 0 || r_off < 0) return *why = "search hit tasks: a negative length or offset", SDF_ERR_INVALID;
  if (n > 0x7fffffffu || len_q > 0x7fffffff || len_r > 0x7fffffff)
    return *why = "search hit tasks: more than 2^31 - 1 hits or bases in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_hit_tasks_host(const sdf_search_hit *hits, size_t n, int64_t len_q, int64_t len_r, int64_t q_off, int q_rc,
                                         int64_t r_off, int r_rc, sdf_filter_task *out) {
  if (n == 0) return SDF_OK;
  const char *why = nullptr;
  if (int rc = hit_tasks_scalars(n, len_q, len_r, q_off, r_off, &why)) return rc;
  if (!hits || !out) return SDF_ERR_INVALID;
  const FilterTaskArgs A{len_q, len_r, q_off, r_off, 0, q_rc != 0, r_rc != 0, 0};
  for (size_t t = 0; t < n; t++) out[t] = hit_task_of(A, hits[t]);
  return SDF_OK;
}

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
