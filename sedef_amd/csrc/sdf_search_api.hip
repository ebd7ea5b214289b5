// The C ABI: the device and uploading forms of search seeding, the reference intervals of every query window
// (search_seeds.hip), of the roll of every interval to its best initial match (search_roll.hip) and of the extension of every
// rolled interval to its hit (search_extend.hip, search_extend_long.hip), with their launches.  The `_host` forms, the
// per-item rules with which the uploading forms complete what the kernels leave, and the checks: search_host.hip.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "sdf_entry.h"
#include "search_host.h"

using namespace sdf;

// What sdf_search_windows_wide_device adds to a call: the list's room, and where the caller wants the number of eligible windows.
struct WideRun {
  size_t n_max;
  uint64_t *d_total;
};
template <bool EMIT>
static void wide_launch(sdf_ctx *ctx, const WideRun &wide, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r,
                        int32_t init_len, int same_genome, const int32_t *d_limit, size_t n_limit, sdf_search_window *d_windows,
                        const uint64_t *d_first, sdf_search_interval *d_out, size_t cap, hipStream_t st, const FoundIndex *F) {
  const auto kernel = F ? search_window_wide_kernel<EMIT, true> : search_window_wide_kernel<EMIT, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)wide.n_max), dim3(SEARCH_WIDE_THREADS), 0, st, d_q, (int)nq, (long long)len_q, d_r,
                     (const SearchLook *)ctx->sw_look.p, (int)init_len, same_genome, d_limit, (int)n_limit, d_windows, (uint32_t *)ctx->sw_counts.p,
                     d_first, d_out, (uint64_t)cap, F ? *F : FoundIndex{}, (const uint32_t *)ctx->sw_wide.p,
                     (const unsigned long long *)ctx->sw_nwide.p, (uint32_t)wide.n_max);
  ctx->launches += 1;
}

// The launches in front of the intervals, on `st`: keys, their sort, prev, lookup, the windows' records and counts (wide: the list
// and the listed windows' records and counts behind them), d_first.
static int search_count(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r, size_t nr,
                        uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *d_limit, size_t n_limit,
                        uint64_t *d_first, sdf_search_window *d_windows, hipStream_t st, const FoundIndex *F = nullptr,
                        const WideRun *wide = nullptr) {
  const int n = (int)nq;
  if (wide) {
    SDF_HIP(ctx->sw_wide.reserve(wide->n_max * 4));
    SDF_HIP(ctx->sw_nwide.reserve(8));
  }
  SDF_HIP(ctx->sw_keys.reserve(2 * nq * 8));
  SDF_HIP(ctx->sw_vals.reserve(2 * nq * 4));
  SDF_HIP(ctx->sw_look.reserve(nq * sizeof(SearchLook)));
  SDF_HIP(ctx->sw_counts.reserve(nq * 4));
  unsigned long long *d_keys = (unsigned long long *)ctx->sw_keys.p, *d_keys2 = d_keys + nq;
  uint32_t *d_vals = (uint32_t *)ctx->sw_vals.p, *d_vals2 = d_vals + nq;
  SearchLook *d_look = (SearchLook *)ctx->sw_look.p;
  uint32_t *d_counts = (uint32_t *)ctx->sw_counts.p;
  size_t t_pairs = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_pairs, d_keys, d_keys2, d_vals, d_vals2, n, 0, 64, st));
  SDF_HIP(ctx->sw_tmp.reserve(t_pairs + 256));
  const dim3 grid((unsigned)((nq + 255) / 256)), block(256);
  hipLaunchKernelGGL(search_keys_kernel, grid, block, 0, st, d_q, n, d_keys, d_vals);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->sw_tmp.p, t_pairs, d_keys, d_keys2, d_vals, d_vals2, n, 0, 64, st));
  hipLaunchKernelGGL(search_prev_kernel, grid, block, 0, st, d_keys2, d_vals2, n, d_look);
  hipLaunchKernelGGL(search_lookup_kernel, grid, block, 0, st, d_q, n, d_r, (int)nr, r_threshold, (int)init_len, uppercase_seeds, d_look);
  const auto kernel = F ? search_window_kernel<false, true> : search_window_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(64), 0, st, d_q, n, (long long)len_q, d_r, (const SearchLook *)d_look, (int)init_len,
                     same_genome, d_limit, (int)n_limit, d_windows, d_counts, (const uint64_t *)nullptr, (sdf_search_interval *)nullptr,
                     (uint64_t)0, F ? *F : FoundIndex{});
  if (wide) {
    hipLaunchKernelGGL(search_wide_list_kernel, dim3(1), dim3(1024), 0, st, (const sdf_search_window *)d_windows, n, (uint32_t)wide->n_max,
                       (uint32_t *)ctx->sw_wide.p, (unsigned long long *)ctx->sw_nwide.p, (unsigned long long *)wide->d_total);
    ctx->launches += 1;
    wide_launch<false>(ctx, *wide, d_q, nq, len_q, d_r, init_len, same_genome, d_limit, n_limit, d_windows, nullptr, nullptr, 0, st, F);
  }
  hipLaunchKernelGGL(stats_cuts_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, n, d_first);
  SDF_HIP(hipGetLastError());
  ctx->launches += 5;
  return SDF_OK;
}
// the intervals (after search_count on the same stream)
static int search_emit(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r, int32_t init_len,
                       int same_genome, const int32_t *d_limit, size_t n_limit, const uint64_t *d_first, sdf_search_interval *d_out,
                       size_t cap, hipStream_t st, const FoundIndex *F = nullptr, const WideRun *wide = nullptr) {
  const auto kernel = F ? search_window_kernel<true, true> : search_window_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(64), 0, st, d_q, (int)nq, (long long)len_q, d_r,
                     (const SearchLook *)ctx->sw_look.p, (int)init_len, same_genome, d_limit, (int)n_limit, (sdf_search_window *)nullptr,
                     (uint32_t *)nullptr, d_first, d_out, (uint64_t)cap, F ? *F : FoundIndex{});
  ctx->launches += 1;
  if (wide) wide_launch<true>(ctx, *wide, d_q, nq, len_q, d_r, init_len, same_genome, d_limit, n_limit, nullptr, d_first, d_out, cap, st, F);
  SDF_HIP(hipGetLastError());
  return SDF_OK;
}

// sdf_search_windows_device, and with_found sdf_search_windows_found_device (a list without a record runs the plain kernels);
// n_wide_max > 0: sdf_search_windows_wide_device
static int windows_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted, size_t nr,
                          uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *d_limit, size_t n_limit,
                          bool with_found, const sdf_search_found *d_found, size_t nf, size_t found_entries_cap, uint64_t *d_found_entries,
                          const uint32_t *d_visible, uint64_t *d_first, sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap,
                          size_t *used, void *stream, size_t n_wide_max = 0, uint64_t *d_wide_total = nullptr) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0) {
    if (used) *used = 0;
    return SDF_OK;
  }
  if (!d_q || !d_first || !d_windows || (cap && !d_out) || (nr && !d_r_sorted) || (n_limit && !d_limit) ||
      (with_found && ((nf && !d_found) || !d_visible)))
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_windows_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = search_scalars(nq, nr, init_len, n_limit, &why)) return refuse(ctx, rc, why);
  if (with_found)
    if (int rc = found_scalars(nf, found_entries_cap, &why)) return refuse(ctx, rc, why);
  if (n_wide_max > SEARCH_WIDE_MAX_LIST) return refuse(ctx, SDF_ERR_UNSUPPORTED, "sdf_search_windows_wide_device: n_wide_max > 2^20");
  const WideRun wide{n_wide_max, d_wide_total}, *Wp = n_wide_max ? &wide : nullptr;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  FoundIndex F{};
  if (with_found)
    if (int rc = found_index(ctx, d_found, nf, found_entries_cap, d_found_entries, d_visible, st, &F)) return rc;
  const FoundIndex *Fp = with_found && nf ? &F : nullptr;
  if (int rc = search_count(ctx, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, d_limit,
                            n_limit, d_first, d_windows, st, Fp, Wp))
    return rc;
  if (int rc = search_emit(ctx, d_q, nq, len_q, d_r_sorted, init_len, same_genome != 0, d_limit, n_limit, d_first, d_out, cap, st, Fp, Wp)) return rc;
  if (stream) return SDF_OK;
  const int rc = counted_need(ctx, d_first, nq, nullptr, st, cap, used, "the windows have ", " intervals, more than cap");
  if (rc == SDF_ERR_HIP || !with_found) return rc;
  // (an index that did not fit comes first: the intervals counted on it are not the answer)
  if (int short_index = found_index_need(ctx, found_entries_cap)) return short_index;
  return rc;
}

extern "C" int sdf_search_windows_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted,
                                         size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                         const int32_t *d_limit, size_t n_limit, uint64_t *d_first, sdf_search_window *d_windows,
                                         sdf_search_interval *d_out, size_t cap, size_t *used, void *stream) {
  return windows_device(ctx, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit, n_limit, false,
                        nullptr, 0, 0, nullptr, nullptr, d_first, d_windows, d_out, cap, used, stream);
}

extern "C" int sdf_search_windows_found_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q,
                                               const sdf_minimizer *d_r_sorted, size_t nr, uint32_t r_threshold, int32_t init_len,
                                               int same_genome, int uppercase_seeds, const int32_t *d_limit, size_t n_limit,
                                               const sdf_search_found *d_found, size_t nf, size_t found_entries_cap,
                                               uint64_t *d_found_entries, const uint32_t *d_visible, uint64_t *d_first,
                                               sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap, size_t *used,
                                               void *stream) {
  return windows_device(ctx, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit, n_limit, true,
                        d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows, d_out, cap, used, stream);
}

extern "C" int sdf_search_windows_wide_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted,
                                              size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                              const int32_t *d_limit, size_t n_limit, const sdf_search_found *d_found, size_t nf,
                                              size_t found_entries_cap, uint64_t *d_found_entries, const uint32_t *d_visible,
                                              uint64_t *d_first, sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap,
                                              size_t *used, size_t n_wide_max, uint64_t *d_wide_total, void *stream) {
  // (no record and no prefixes: the plain form, without an index)
  return windows_device(ctx, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit, n_limit,
                        nf != 0 || d_visible != nullptr, d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows, d_out, cap,
                        used, stream, n_wide_max, d_wide_total);
}

// sdf_search_windows, and with_found sdf_search_windows_found: the device form on copies, what it left completed on the host
static int windows_checked(sdf_ctx *ctx, const SearchArgs &A, bool with_found, const sdf_search_found *found, size_t nf,
                           const uint32_t *visible, uint64_t *first, sdf_search_window *windows, sdf_search_interval *out, size_t cap,
                           size_t *used) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const size_t nq = A.nq, nr = A.nr, n_limit = A.n_limit;
  const sdf_minimizer *q = A.q, *r_sorted = A.r;
  const int32_t *limit = A.limit;
  const int64_t len_q = A.len_q;
  const int32_t init_len = A.init_len;
  if (nq == 0) {
    if (used) *used = 0;
    if (first) first[0] = 0;
    return SDF_OK;
  }
  const char *why = nullptr;
  if (int rc = search_arrays(A, first, windows, out, cap, used, &why)) return refuse(ctx, rc, why);
  uint64_t entries = 0;
  if (with_found)
    if (int rc = found_arrays(found, nf, visible, nq, &entries, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  FoundIndex F{};
  const FoundIndex *Fp = nullptr;
  if (with_found && nf) {
    if (int rc = upload_all(ctx, st, {{ctx->fo_found, found, nf * sizeof(sdf_search_found)}, {ctx->fo_vis, visible, nq * 4}})) return rc;
    if (int rc = found_index(ctx, (const sdf_search_found *)ctx->fo_found.p, nf, (size_t)entries, nullptr, (const uint32_t *)ctx->fo_vis.p, st, &F))
      return rc;
    Fp = &F;
  }
  if (int rc = upload_all(ctx, st, {{ctx->sw_q, q, nq * sizeof(sdf_minimizer)}, {ctx->sw_r, r_sorted, nr * sizeof(sdf_minimizer)},
                                   {ctx->sw_limit, limit, n_limit * 4}}))
    return rc;
  SDF_HIP(ctx->sw_first.reserve((nq + 1) * 8));
  SDF_HIP(ctx->sw_win.reserve(nq * sizeof(sdf_search_window)));
  const sdf_minimizer *d_q = (const sdf_minimizer *)ctx->sw_q.p, *d_r = (const sdf_minimizer *)ctx->sw_r.p;
  const int32_t *d_limit = (const int32_t *)ctx->sw_limit.p;
  uint64_t *d_first = (uint64_t *)ctx->sw_first.p;
  if (int rc = search_count(ctx, d_q, nq, len_q, d_r, nr, A.r_threshold, init_len, A.same_genome, A.uppercase_seeds, d_limit, n_limit, d_first,
                            (sdf_search_window *)ctx->sw_win.p, st, Fp))
    return rc;
  SDF_HIP(hipMemcpyAsync(windows, ctx->sw_win.p, nq * sizeof(sdf_search_window), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(first, d_first, (nq + 1) * 8, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  const uint64_t dev_need = first[nq];
  // the WIDE (and FOUND_WIDE) windows, on the host; their intervals in window order, wide_first[t] those of the wide windows before the t-th
  std::vector<size_t> wide;
  std::vector<uint64_t> wide_first(1, 0);
  std::vector<sdf_search_interval> T;
  SearchScratch S;
  for (size_t i = 0; i < nq; i++) {
    if (!(windows[i].flags & (SDF_SEARCH_WIDE | SDF_SEARCH_FOUND_WIDE))) continue;
    const FoundView V{found, with_found ? (size_t)visible[i] : 0};
    search_one_window(A, i, windows[i], T, S, with_found ? &V : nullptr);
    wide.push_back(i);
    wide_first.push_back(T.size());
  }
  const uint64_t need = dev_need + T.size();
  *used = (size_t)need;
  if (!wide.empty()) {  // first[] with the wide windows' intervals in it
    size_t t = 0;
    for (size_t i = 0; i <= nq; i++) {
      while (t < wide.size() && wide[t] < i) ++t;
      first[i] += wide_first[t];
    }
  }
  if (need > cap) return refuse(ctx, SDF_ERR_CIGAR_OVERFLOW, "the windows have " + std::to_string(need) + " intervals, more than cap");
  if (dev_need) {
    SDF_HIP(ctx->sw_out.reserve((size_t)dev_need * sizeof(sdf_search_interval)));
    if (int rc = search_emit(ctx, d_q, nq, len_q, d_r, init_len, A.same_genome, d_limit, n_limit, d_first, (sdf_search_interval *)ctx->sw_out.p,
                             (size_t)dev_need, st, Fp))
      return rc;
    SDF_HIP(hipMemcpyAsync(out, ctx->sw_out.p, (size_t)dev_need * sizeof(sdf_search_interval), hipMemcpyDeviceToHost, st));
    SDF_HIP(hipStreamSynchronize(st));
  }
  // make room for the wide windows' intervals: from the last wide window down, what lies behind it moves up by what precedes it
  uint64_t dev_end = dev_need;  // the device's records [.., dev_end) have not moved yet
  for (size_t t = wide.size(); t-- > 0;) {
    const size_t i = wide[t];
    const uint64_t dev_at = first[i] - wide_first[t];  // where the device's records of the windows behind i begin
    memmove(out + first[i + 1], out + dev_at, (size_t)(dev_end - dev_at) * sizeof(sdf_search_interval));
    memcpy(out + first[i], T.data() + wide_first[t], (size_t)(wide_first[t + 1] - wide_first[t]) * sizeof(sdf_search_interval));
    dev_end = dev_at;
  }
  return SDF_OK;
}

extern "C" int sdf_search_windows(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                                  uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *limit,
                                  size_t n_limit, uint64_t *first, sdf_search_window *windows, sdf_search_interval *out, size_t cap,
                                  size_t *used) {
  const SearchArgs A{q, nq, len_q, r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, limit, n_limit};
  return windows_checked(ctx, A, false, nullptr, 0, nullptr, first, windows, out, cap, used);
}

extern "C" int sdf_search_windows_found(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted,
                                        size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                        const int32_t *limit, size_t n_limit, const sdf_search_found *found, size_t nf,
                                        const uint32_t *visible, uint64_t *first, sdf_search_window *windows, sdf_search_interval *out,
                                        size_t cap, size_t *used) {
  const SearchArgs A{q, nq, len_q, r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, limit, n_limit};
  return windows_checked(ctx, A, true, found, nf, visible, first, windows, out, cap, used);
}

// ---- the roll ----

namespace {
// the launch: n wavefronts on `st`
template <bool WALK>
int roll_launch(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows, const uint64_t *d_first,
                const sdf_search_interval *d_intervals, size_t n, const sdf_minimizer *d_r, size_t nr, int64_t len_r, int32_t init_len,
                const int32_t *d_limit, size_t n_limit, sdf_search_roll_rec *d_out, hipStream_t st) {
  hipLaunchKernelGGL(search_roll_kernel<WALK>, dim3((unsigned)n), dim3(64), 0, st, d_q, (int)nq, d_windows, d_first, d_intervals, d_r, (int)nr,
                     (long long)len_r, (int)init_len, d_limit, (int)n_limit, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}

int roll_device(sdf_ctx *ctx, bool walk, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows, const uint64_t *d_first,
                const sdf_search_interval *d_intervals, size_t n_max, const sdf_minimizer *d_r, size_t nr, int64_t len_r, int32_t init_len,
                const int32_t *d_limit, size_t n_limit, sdf_search_roll_rec *d_out, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0 || n_max == 0) return SDF_OK;
  if (!d_q || !d_windows || !d_first || !d_intervals || !d_r || !d_limit || !d_out)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_roll_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = roll_scalars(nq, n_max, nr, len_r, init_len, n_limit, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (int rc = walk ? roll_launch<true>(ctx, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, len_r, init_len, d_limit, n_limit, d_out, st)
                    : roll_launch<false>(ctx, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, len_r, init_len, d_limit, n_limit, d_out, st))
    return rc;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_roll_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                      const uint64_t *d_first, const sdf_search_interval *d_intervals, size_t n_max, const sdf_minimizer *d_r,
                                      size_t nr, int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                                      sdf_search_roll_rec *d_out, void *stream) {
  return roll_device(ctx, true, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, len_r, init_len, d_limit, n_limit, d_out, stream);
}

// For profiles/search_roll.py, not in the header: the device form whose wavefronts leave after the set-up (gather, sort, slots),
// so that its time against the whole call's is the walk's share.  d_out's records are NOT the intervals'.
extern "C" int sdf_search_roll_setup_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                            const uint64_t *d_first, const sdf_search_interval *d_intervals, size_t n_max,
                                            const sdf_minimizer *d_r, size_t nr, int64_t len_r, int32_t init_len, const int32_t *d_limit,
                                            size_t n_limit, sdf_search_roll_rec *d_out, void *stream) {
  return roll_device(ctx, false, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, len_r, init_len, d_limit, n_limit, d_out, stream);
}

extern "C" int sdf_search_roll(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                               const sdf_search_interval *intervals, const sdf_minimizer *r, size_t nr, int64_t len_r, int32_t init_len,
                               const int32_t *limit, size_t n_limit, sdf_search_roll_rec *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0) return SDF_OK;
  const RollArgs A{q, nq, windows, first, intervals, r, nr, len_r, init_len, limit, n_limit};
  const char *why = nullptr;
  if (int rc = roll_arrays(A, out, &why)) return refuse(ctx, rc, why);
  const size_t n = (size_t)first[nq];
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_all(ctx, st, {{ctx->sr_q, q, nq * sizeof(sdf_minimizer)}, {ctx->sr_win, windows, nq * sizeof(sdf_search_window)},
                                   {ctx->sr_first, first, (nq + 1) * 8}, {ctx->sr_iv, intervals, n * sizeof(sdf_search_interval)},
                                   {ctx->sr_r, r, nr * sizeof(sdf_minimizer)}, {ctx->sr_limit, limit, n_limit * 4}}))
    return rc;
  SDF_HIP(ctx->sr_out.reserve(n * sizeof(sdf_search_roll_rec)));
  if (int rc = roll_launch<true>(ctx, (const sdf_minimizer *)ctx->sr_q.p, nq, (const sdf_search_window *)ctx->sr_win.p,
                                 (const uint64_t *)ctx->sr_first.p, (const sdf_search_interval *)ctx->sr_iv.p, n,
                                 (const sdf_minimizer *)ctx->sr_r.p, nr, len_r, init_len, (const int32_t *)ctx->sr_limit.p, n_limit,
                                 (sdf_search_roll_rec *)ctx->sr_out.p, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->sr_out.p, n * sizeof(sdf_search_roll_rec), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  // the WIDE intervals, on the host
  ExtendMap M;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++)
      if (out[t].flags & SDF_ROLL_WIDE) roll_one(A, i, intervals[t], out[t], M);
  return SDF_OK;
}

// ---- the extension ----

namespace {
int extend_launch(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows, const uint64_t *d_first,
                  const sdf_search_interval *d_intervals, const sdf_search_roll_rec *d_rolls, const sdf_filter_rec *d_filter, size_t n,
                  const sdf_minimizer *d_r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                  const sdf_extend_params &P, sdf_search_hit *d_out, hipStream_t st) {
  hipLaunchKernelGGL(search_extend_kernel, dim3((unsigned)n), dim3(64), 0, st, d_q, (int)nq, d_windows, d_first, d_intervals, d_rolls, d_filter,
                     d_r, (int)nr, (long long)len_q, (long long)len_r, (int)init_len, d_limit, (int)n_limit, P, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_extend_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                        const uint64_t *d_first, const sdf_search_interval *d_intervals, const sdf_search_roll_rec *d_rolls,
                                        const sdf_filter_rec *d_filter, size_t n_max, const sdf_minimizer *d_r, size_t nr, int64_t len_q,
                                        int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                                        const sdf_extend_params *params, sdf_search_hit *d_out, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0 || n_max == 0) return SDF_OK;
  if (!d_q || !d_windows || !d_first || !d_intervals || !d_rolls || !d_r || !d_limit || !d_out)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_extend_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = roll_scalars(nq, n_max, nr, len_r, init_len, n_limit, &why)) return refuse(ctx, rc, why);
  if (int rc = extend_scalars(len_q, params, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (int rc = extend_launch(ctx, d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, n_max, d_r, nr, len_q, len_r, init_len, d_limit,
                             n_limit, *params, d_out, st))
    return rc;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// ---- the extension, long form (search_extend_long.hip) ----

namespace {
constexpr size_t kExtendLongBatch = 128;  // batch slots by default: 128 * 69,632 entries of 32 bytes are 272 MiB at the largest long_grow
constexpr size_t kExtendLongMaxBatch = 4096;

// The workspace of a call and the launches that fill it.  Everything here follows from n_max, n_long_max, the stride (ext_long_args) and batch.
struct ExtendLongPlan {
  size_t batch, stride, items, batches;
  size_t off_flag, off_pos, off_list, off_meta, off_nds, off_keys, off_keys2, off_vals, off_vals2, off_incl, off_slots, bytes, tmp_bytes;
  int end_bit;
};
int extend_long_plan(sdf_ctx *ctx, size_t n_max, size_t n_long_max, int stride, size_t batch, ExtendLongPlan &L, hipStream_t st) {
  L.batch = std::min(std::min(batch ? batch : kExtendLongBatch, kExtendLongMaxBatch), n_long_max);
  L.stride = (size_t)stride;
  L.items = L.batch * L.stride;
  L.batches = (n_long_max + L.batch - 1) / L.batch;
  size_t at = 0;
  const auto take = [&](size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  L.off_flag = take((n_max + 1) * 4), L.off_pos = take((n_max + 1) * 4), L.off_list = take(n_long_max * sizeof(ExtLongCand));
  L.off_meta = take(16), L.off_nds = take(L.batch * 4);
  L.off_keys = take(L.items * 8), L.off_keys2 = take(L.items * 8), L.off_vals = take(L.items * 4), L.off_vals2 = take(L.items * 4);
  L.off_incl = take(L.items * 4), L.off_slots = take(L.items * 4);
  L.bytes = at;
  L.end_bit = kLongSlotShift;
  while (((size_t)1 << (L.end_bit - kLongSlotShift)) < L.batch) ++L.end_bit;
  size_t t_sort = 0, t_scan = 0, t_sel = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)L.items, 0, L.end_bit, st));
  SDF_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, t_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)L.items, st));
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_sel, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(n_max + 1), st));
  L.tmp_bytes = std::max(t_sort, std::max(t_scan, t_sel)) + 256;
  return SDF_OK;
}

// what the long form's launches share; its stride, the universe entries a batch slot owns, follows from grow
ExtLongArgs ext_long_args(const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows, const uint64_t *d_first,
                          const sdf_search_interval *d_intervals, const sdf_search_roll_rec *d_rolls, const sdf_filter_rec *d_filter,
                          const sdf_minimizer *d_r, size_t nr, size_t n_limit, int32_t grow) {
  return ExtLongArgs{d_q, d_r, d_windows, d_first, d_intervals, d_rolls, d_filter, (int)nq, (int)nr, (int)n_limit, (int)grow,
                     SDF_SEARCH_MAX_MEMBERS + SDF_ROLL_MAX_SPAN + 4 * (int)grow};
}

// the launches, on `st`; d_left or null
int extend_long_run(sdf_ctx *ctx, const ExtLongArgs &A, size_t n_max, size_t n_long_max, size_t batch, int64_t len_q, int64_t len_r,
                    int32_t init_len, const int32_t *d_limit, const sdf_extend_params &P, sdf_search_hit *d_hits, uint64_t *d_left, hipStream_t st) {
  ExtendLongPlan L;
  if (int rc = extend_long_plan(ctx, n_max, n_long_max, A.stride, batch, L, st)) return rc;
  if (L.items > 0x7fffffffu) return refuse(ctx, SDF_ERR_UNSUPPORTED, "search extend, long form: a batch of more than 2^31 - 1 universe entries");
  if (L.bytes + L.tmp_bytes > ctx->ws_budget || ctx->sl_ws.reserve(L.bytes) != hipSuccess || ctx->sl_tmp.reserve(L.tmp_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return refuse(ctx, SDF_ERR_NOMEM, "search extend, long form: " + std::to_string((L.bytes + L.tmp_bytes) >> 20) + " MiB of workspace cannot be had (a smaller batch needs less)");
  }
  uint8_t *ws = (uint8_t *)ctx->sl_ws.p;
  uint32_t *d_flag = (uint32_t *)(ws + L.off_flag), *d_pos = (uint32_t *)(ws + L.off_pos), *d_meta = (uint32_t *)(ws + L.off_meta);
  uint32_t *d_nds = (uint32_t *)(ws + L.off_nds), *d_vals = (uint32_t *)(ws + L.off_vals), *d_vals2 = (uint32_t *)(ws + L.off_vals2);
  uint32_t *d_incl = (uint32_t *)(ws + L.off_incl), *d_slots = (uint32_t *)(ws + L.off_slots), *d_heads = d_vals;  // (the payloads are sorted by then)
  ExtLongCand *d_list = (ExtLongCand *)(ws + L.off_list);
  unsigned long long *d_keys = (unsigned long long *)(ws + L.off_keys), *d_keys2 = (unsigned long long *)(ws + L.off_keys2);
  const int n = (int)n_max, items = (int)L.items, stride = (int)L.stride;
  const dim3 block(256), grid_n((unsigned)((n_max + 1 + 255) / 256)), grid_items((unsigned)((L.items + 255) / 256));
  size_t tmp = L.tmp_bytes;
  hipLaunchKernelGGL(search_extend_long_flag_kernel, grid_n, block, 0, st, A, (const sdf_search_hit *)d_hits, n, d_flag);
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->sl_tmp.p, tmp, d_flag, d_pos, n + 1, st));
  hipLaunchKernelGGL(search_extend_long_list_kernel, grid_n, block, 0, st, A, (const sdf_search_hit *)d_hits, (const uint32_t *)d_flag,
                     (const uint32_t *)d_pos, n, (uint32_t)n_long_max, d_list, d_meta, (unsigned long long *)d_left);
  ctx->launches += 3;
  for (size_t b = 0; b < L.batches; b++) {
    const uint32_t base = (uint32_t)(b * L.batch);
    hipLaunchKernelGGL(search_extend_long_keys_kernel, dim3((unsigned)((L.stride + 255) / 256), (unsigned)L.batch), block, 0, st, A,
                       (const ExtLongCand *)d_list, (const uint32_t *)d_meta, base, d_keys, d_vals);
    tmp = L.tmp_bytes;
    SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->sl_tmp.p, tmp, d_keys, d_keys2, d_vals, d_vals2, items, 0, L.end_bit, st));
    hipLaunchKernelGGL(search_extend_long_heads_kernel, grid_items, block, 0, st, (const unsigned long long *)d_keys2, items, stride, d_heads);
    tmp = L.tmp_bytes;
    SDF_HIP(hipcub::DeviceScan::InclusiveSum(ctx->sl_tmp.p, tmp, d_heads, d_incl, items, st));
    hipLaunchKernelGGL(search_extend_long_slots_kernel, grid_items, block, 0, st, (const unsigned long long *)d_keys2, (const uint32_t *)d_vals2,
                       (const uint32_t *)d_incl, items, stride, d_slots, d_nds);
    hipLaunchKernelGGL(search_extend_long_kernel, dim3((unsigned)L.batch), dim3(64), 0, st, A, (const ExtLongCand *)d_list, (const uint32_t *)d_meta,
                       base, (const uint32_t *)d_slots, (const uint32_t *)d_nds, (long long)len_q, (long long)len_r, (int)init_len, d_limit, P,
                       d_hits, (unsigned long long *)d_left);
    ctx->launches += 6;
  }
  SDF_HIP(hipGetLastError());
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_extend_long_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                             const uint64_t *d_first, const sdf_search_interval *d_intervals,
                                             const sdf_search_roll_rec *d_rolls, const sdf_filter_rec *d_filter, size_t n_max,
                                             const sdf_minimizer *d_r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len,
                                             const int32_t *d_limit, size_t n_limit, const sdf_extend_params *params, int32_t long_grow,
                                             size_t n_long_max, size_t batch, sdf_search_hit *d_hits, uint64_t *d_left, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0 || n_max == 0 || n_long_max == 0) return SDF_OK;
  if (!d_q || !d_windows || !d_first || !d_intervals || !d_rolls || !d_r || !d_limit || !d_hits)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_extend_long_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = roll_scalars(nq, n_max, nr, len_r, init_len, n_limit, &why)) return refuse(ctx, rc, why);
  if (int rc = extend_scalars(len_q, params, &why)) return refuse(ctx, rc, why);
  if (long_grow <= SDF_EXTEND_MAX_GROW || long_grow > SDF_EXTEND_LONG_MAX_GROW)
    return refuse(ctx, SDF_ERR_INVALID, "search extend, long form: long_grow outside SDF_EXTEND_MAX_GROW + 1 .. SDF_EXTEND_LONG_MAX_GROW");
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const ExtLongArgs A = ext_long_args(d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, d_r, nr, n_limit, long_grow);
  if (int rc = extend_long_run(ctx, A, n_max, std::min(n_long_max, n_max), batch, len_q, len_r, init_len, d_limit, *params, d_hits, d_left, st)) return rc;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_search_extend(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                 const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, const sdf_filter_rec *filter,
                                 const sdf_minimizer *r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *limit,
                                 size_t n_limit, const sdf_extend_params *params, sdf_search_hit *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0) return SDF_OK;
  const RollArgs RA{q, nq, windows, first, intervals, r, nr, len_r, init_len, limit, n_limit};
  const char *why = nullptr;
  if (int rc = roll_arrays(RA, out, &why)) return refuse(ctx, rc, why);
  const size_t n = (size_t)first[nq];
  if (n == 0) return SDF_OK;
  if (!rolls) return refuse(ctx, SDF_ERR_INVALID, "search extend: invalid arguments");
  if (int rc = extend_scalars(len_q, params, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_all(ctx, st, {{ctx->sr_q, q, nq * sizeof(sdf_minimizer)}, {ctx->sr_win, windows, nq * sizeof(sdf_search_window)},
                                   {ctx->sr_first, first, (nq + 1) * 8}, {ctx->sr_iv, intervals, n * sizeof(sdf_search_interval)},
                                   {ctx->sr_r, r, nr * sizeof(sdf_minimizer)}, {ctx->sr_limit, limit, n_limit * 4},
                                   {ctx->se_rolls, rolls, n * sizeof(sdf_search_roll_rec)},
                                   {ctx->se_filter, filter, filter ? n * sizeof(sdf_filter_rec) : 0}}))
    return rc;
  SDF_HIP(ctx->se_out.reserve(n * sizeof(sdf_search_hit)));
  if (int rc = extend_launch(ctx, (const sdf_minimizer *)ctx->sr_q.p, nq, (const sdf_search_window *)ctx->sr_win.p,
                             (const uint64_t *)ctx->sr_first.p, (const sdf_search_interval *)ctx->sr_iv.p,
                             (const sdf_search_roll_rec *)ctx->se_rolls.p, filter ? (const sdf_filter_rec *)ctx->se_filter.p : nullptr, n,
                             (const sdf_minimizer *)ctx->sr_r.p, nr, len_q, len_r, init_len, (const int32_t *)ctx->sr_limit.p, n_limit, *params,
                             (sdf_search_hit *)ctx->se_out.p, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->se_out.p, n * sizeof(sdf_search_hit), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  // the intervals that are WIDE for their growth, by the long form on the arrays that are there already
  size_t n_long = 0;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++) {
      if (out[t].flags != SDF_EXTEND_WIDE) continue;
      n_long += !extend_replay_wide(rolls[t], windows[i].n_members, (long long)first_at_or_after(r, nr, intervals[t].start));
    }
  if (n_long) {
    const ExtLongArgs LA = ext_long_args((const sdf_minimizer *)ctx->sr_q.p, nq, (const sdf_search_window *)ctx->sr_win.p,
                                         (const uint64_t *)ctx->sr_first.p, (const sdf_search_interval *)ctx->sr_iv.p,
                                         (const sdf_search_roll_rec *)ctx->se_rolls.p, filter ? (const sdf_filter_rec *)ctx->se_filter.p : nullptr,
                                         (const sdf_minimizer *)ctx->sr_r.p, nr, n_limit, SDF_EXTEND_LONG_MAX_GROW);
    // (no room for the default batch's workspace: smaller batches -- more launches, less in flight -- before the host takes over)
    int rc = SDF_ERR_NOMEM;
    for (size_t batch = kExtendLongBatch; rc == SDF_ERR_NOMEM && batch; batch /= 4)
      rc = extend_long_run(ctx, LA, n, n_long, batch, len_q, len_r, init_len, (const int32_t *)ctx->sr_limit.p, *params,
                           (sdf_search_hit *)ctx->se_out.p, nullptr, st);
    if (rc == SDF_OK) {
      SDF_HIP(hipMemcpyAsync(out, ctx->se_out.p, n * sizeof(sdf_search_hit), hipMemcpyDeviceToHost, st));
      SDF_HIP(hipStreamSynchronize(st));
    } else if (rc == SDF_ERR_NOMEM) {
      // not even one interval's workspace: the host completes them, as it does those beyond the long cap; sdf_last_error() says so
      ctx->err = "sdf_search_extend: no workspace for the long form, " + std::to_string(n_long) + " intervals completed on the host (" + ctx->err + ")";
    } else {
      return rc;
    }
  }
  // what is still WIDE and nobody completed -- the replay does not fit, or the growth passes the long form's cap --, on the host
  const ExtendArgs A{RA, rolls, filter, len_q, *params};
  ExtendMap S;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++)
      if (out[t].flags == SDF_EXTEND_WIDE && out[t].query_end == 0) extend_one(A, i, t, out[t], S);
  return SDF_OK;
}
