// The C ABI: search seeding, the reference intervals of every query window (search_seeds.hip; include/sedef_hip.h states the
// seven steps), and the roll of every interval to its best initial match (search_roll.hip; the header states its rules).
// sdf_search_windows_host and sdf_search_roll_host are those in plain C++; the host forms complete with them what the kernels leave.
// Behind them the extension of every rolled interval to its hit (search_extend.hip), sdf_search_extend_host likewise.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <map>

#include "sdf_entry.h"

using namespace sdf;

namespace {
struct SearchArgs {
  const sdf_minimizer *q;
  size_t nq;
  int64_t len_q;
  const sdf_minimizer *r;
  size_t nr;
  uint32_t r_threshold;
  int32_t init_len;
  bool same_genome, uppercase_seeds;
  const int32_t *limit;
  size_t n_limit;
};
// the found records one window sees (include/sedef_hip.h, the section of the found records): found[0, visible)
struct FoundView {
  const sdf_search_found *found;
  size_t visible;
};
struct SearchScratch {
  std::vector<uint64_t> keys;
  std::vector<int32_t> cand;
};

inline uint64_t search_host_key(const sdf_minimizer &m) { return (uint64_t)(uint32_t)m.status << 32 | m.hash; }

// what every form checks of its scalars; *why: the refusal's text
int search_scalars(size_t nq, size_t nr, int32_t init_len, size_t n_limit, const char **why) {
  if (init_len < 1) return *why = "search windows: init_len < 1", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search windows implement init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x3fffffffu) return *why = "search windows: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (nr > 0x7fffffffu || n_limit > 0x7fffffffu)
    return *why = "search windows: more than 2^31 - 1 reference records or limit entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the host forms of their arrays
int search_arrays(const SearchArgs &A, const uint64_t *first, const sdf_search_window *windows, const void *out, size_t cap,
                  const size_t *used, const char **why) {
  if (!A.q || !first || !windows || !used || (cap && !out) || (A.nr && !A.r) || (A.n_limit && !A.limit))
    return *why = "search windows: invalid arguments", SDF_ERR_INVALID;
  if (int rc = search_scalars(A.nq, A.nr, A.init_len, A.n_limit, why)) return rc;
  for (size_t s = 1; s < A.n_limit; s++)
    if (A.limit[s] < 1) return *why = "search windows: a limit below 1 (the reference reads candidates[-1] there)", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

// Window i as include/sedef_hip.h states it, step by step: its record, its intervals appended to T.  F: the found records the
// window sees, a linear pass per gathered position (null: an empty tree).
void search_one_window(const SearchArgs &A, size_t i, sdf_search_window &W, std::vector<sdf_search_interval> &T, SearchScratch &S,
                       const FoundView *F = nullptr) {
  W.query_size = W.n_members = W.n_gathered = W.n_candidates = 0, W.flags = 0;
  const int64_t qs = A.q[i].loc;
  if (qs + A.init_len > A.len_q) {  // 1
    W.flags = SDF_SEARCH_SHORT;
    return;
  }
  S.keys.clear();
  S.cand.clear();
  if (F) {
    size_t meet = 0;
    for (size_t f = 0; f < F->visible; f++) meet += found_meets_window(F->found[f], qs, A.init_len);
    if (meet > SDF_SEARCH_MAX_FOUND) W.flags |= SDF_SEARCH_FOUND_WIDE;
  }
  const auto excluded = [&](int64_t loc, int64_t pos) {
    if (!F) return false;
    for (size_t f = 0; f < F->visible; f++)
      if (!found_empty(F->found[f]) && found_covers(F->found[f], loc, pos)) return true;
    return false;
  };
  int64_t gathered = 0;
  size_t j = i;
  const auto key_less = [](const sdf_minimizer &m, uint64_t k) { return search_host_key(m) < k; };
  const auto less_key = [](uint64_t k, const sdf_minimizer &m) { return k < search_host_key(m); };
  for (; j < A.nq && (int64_t)A.q[j].loc - qs <= A.init_len; j++) {  // 2
    const sdf_minimizer &m = A.q[j];
    const uint64_t key = search_host_key(m);
    S.keys.push_back(key);
    if (A.uppercase_seeds && m.status != 0) continue;  // 4
    const sdf_minimizer *g0 = std::lower_bound(A.r, A.r + A.nr, key, key_less), *g1 = std::upper_bound(g0, A.r + A.nr, key, less_key);
    if (g0 == g1 || (uint64_t)(g1 - g0) >= A.r_threshold) continue;
    gathered += g1 - g0;
    for (const sdf_minimizer *p = g0; p < g1; p++)
      if ((!A.same_genome || (int64_t)p->loc >= qs + A.init_len) && !excluded(m.loc, p->loc)) S.cand.push_back(p->loc);
  }
  W.n_members = (int32_t)(j - i);
  W.n_gathered = gathered > 0x7fffffff ? 0x7fffffff : (int32_t)gathered;
  if (W.n_members > SDF_SEARCH_MAX_MEMBERS || gathered > SDF_SEARCH_MAX_GATHER) W.flags |= SDF_SEARCH_WIDE;
  std::sort(S.keys.begin(), S.keys.end());
  W.query_size = (int32_t)(std::unique(S.keys.begin(), S.keys.end()) - S.keys.begin());  // 3
  std::sort(S.cand.begin(), S.cand.end());
  S.cand.erase(std::unique(S.cand.begin(), S.cand.end()), S.cand.end());
  W.n_candidates = (int32_t)S.cand.size();
  if ((size_t)W.query_size >= A.n_limit) {  // 5
    W.flags |= SDF_SEARCH_NOLIMIT;
    return;
  }
  const int64_t L = A.limit[W.query_size], n = (int64_t)S.cand.size();
  const size_t t0 = T.size();
  for (int64_t a = 0; a <= n - L; a++) {  // 6
    const int64_t b = a + L - 1, ca = S.cand[a], cb = S.cand[b];
    if (cb - ca > A.init_len) continue;
    const int64_t x = std::max<int64_t>(0, cb - A.init_len + 1), y = ca + 1;
    if (T.size() > t0 && x < T.back().end) T.back().end = (int32_t)std::max<int64_t>(T.back().end, y);
    else T.push_back({(int32_t)x, (int32_t)y});
  }
  if (A.same_genome) {  // 7
    size_t keep = t0;
    for (size_t t = t0; t < T.size(); t++) {
      sdf_search_interval I = T[t];
      I.start = (int32_t)std::max<int64_t>(I.start, qs + A.init_len);
      if (I.start <= I.end) T[keep++] = I;
    }
    T.resize(keep);
  }
}
}  // namespace

namespace {
// what the forms that take host arrays check of a list of found records and its prefixes (n of them, each at most nf);
// *entries: the bin entries of the list
int found_arrays(const sdf_search_found *found, size_t nf, const uint32_t *visible, size_t n, uint64_t *entries, const char **why) {
  if ((nf && !found) || (n && !visible)) return *why = "search found: invalid arguments", SDF_ERR_INVALID;
  if (nf > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 found records in one call", SDF_ERR_UNSUPPORTED;
  for (size_t t = 0; t < n; t++)
    if (visible[t] > nf) return *why = "search found: a prefix longer than the list", SDF_ERR_INVALID;
  sdf_search_found_entries(found, nf, entries);
  if (*entries > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 bin entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

// sdf_search_windows_host, and with found != nullptr or nf > 0 sdf_search_windows_found_host
int windows_host(const SearchArgs &A, bool with_found, const sdf_search_found *found, size_t nf, const uint32_t *visible, uint64_t *first,
                 sdf_search_window *windows, sdf_search_interval *out, size_t cap, size_t *used) {
  const size_t nq = A.nq;
  if (nq == 0) {
    if (used) *used = 0;
    if (first) first[0] = 0;
    return SDF_OK;
  }
  const char *why = nullptr;
  if (int rc = search_arrays(A, first, windows, out, cap, used, &why)) return rc;
  uint64_t entries = 0;
  if (with_found)
    if (int rc = found_arrays(found, nf, visible, nq, &entries, &why)) return rc;
  // every window once; the intervals are kept here while they still fit below cap and reach `out` only when all of them do
  SearchScratch S;
  std::vector<sdf_search_interval> T, all;
  uint64_t at = 0;
  for (size_t i = 0; i < nq; i++) {
    first[i] = at;
    T.clear();
    const FoundView F{found, with_found ? (size_t)visible[i] : 0};
    search_one_window(A, i, windows[i], T, S, with_found ? &F : nullptr);
    at += T.size();
    if (at <= cap) all.insert(all.end(), T.begin(), T.end());
  }
  first[nq] = at;
  *used = (size_t)at;
  if (at > cap) return SDF_ERR_CIGAR_OVERFLOW;
  if (at) memcpy(out, all.data(), (size_t)at * sizeof(sdf_search_interval));
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_windows_host(const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                                       uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                       const int32_t *limit, size_t n_limit, uint64_t *first, sdf_search_window *windows,
                                       sdf_search_interval *out, size_t cap, size_t *used) {
  const SearchArgs A{q, nq, len_q, r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, limit, n_limit};
  return windows_host(A, false, nullptr, 0, nullptr, first, windows, out, cap, used);
}

extern "C" int sdf_search_windows_found_host(const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                                             uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                             const int32_t *limit, size_t n_limit, const sdf_search_found *found, size_t nf,
                                             const uint32_t *visible, uint64_t *first, sdf_search_window *windows,
                                             sdf_search_interval *out, size_t cap, size_t *used) {
  const SearchArgs A{q, nq, len_q, r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, limit, n_limit};
  return windows_host(A, true, found, nf, visible, first, windows, out, cap, used);
}

// The launches in front of the intervals, on `st`: keys, their sort, prev, lookup, the windows' records and counts, d_first.
static int search_count(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r, size_t nr,
                        uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *d_limit, size_t n_limit,
                        uint64_t *d_first, sdf_search_window *d_windows, hipStream_t st, const FoundIndex *F = nullptr) {
  const int n = (int)nq;
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
  hipLaunchKernelGGL(stats_cuts_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, n, d_first);
  SDF_HIP(hipGetLastError());
  ctx->launches += 5;
  return SDF_OK;
}
// the intervals (after search_count on the same stream)
static int search_emit(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r, int32_t init_len,
                       int same_genome, const int32_t *d_limit, size_t n_limit, const uint64_t *d_first, sdf_search_interval *d_out,
                       size_t cap, hipStream_t st, const FoundIndex *F = nullptr) {
  const auto kernel = F ? search_window_kernel<true, true> : search_window_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(64), 0, st, d_q, (int)nq, (long long)len_q, d_r,
                     (const SearchLook *)ctx->sw_look.p, (int)init_len, same_genome, d_limit, (int)n_limit, (sdf_search_window *)nullptr,
                     (uint32_t *)nullptr, d_first, d_out, (uint64_t)cap, F ? *F : FoundIndex{});
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}

// sdf_search_windows_device, and with_found sdf_search_windows_found_device (a list without a record runs the plain kernels)
static int windows_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted, size_t nr,
                          uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *d_limit, size_t n_limit,
                          bool with_found, const sdf_search_found *d_found, size_t nf, size_t found_entries_cap, uint64_t *d_found_entries,
                          const uint32_t *d_visible, uint64_t *d_first, sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap,
                          size_t *used, void *stream) {
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
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  FoundIndex F{};
  if (with_found)
    if (int rc = found_index(ctx, d_found, nf, found_entries_cap, d_found_entries, d_visible, st, &F)) return rc;
  const FoundIndex *Fp = with_found && nf ? &F : nullptr;
  if (int rc = search_count(ctx, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome != 0, uppercase_seeds != 0, d_limit,
                            n_limit, d_first, d_windows, st, Fp))
    return rc;
  if (int rc = search_emit(ctx, d_q, nq, len_q, d_r_sorted, init_len, same_genome != 0, d_limit, n_limit, d_first, d_out, cap, st, Fp)) return rc;
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
    SDF_HIP(ctx->fo_found.reserve(nf * sizeof(sdf_search_found)));
    SDF_HIP(ctx->fo_vis.reserve(nq * 4));
    SDF_HIP(hipMemcpyAsync(ctx->fo_found.p, found, nf * sizeof(sdf_search_found), hipMemcpyHostToDevice, st));
    SDF_HIP(hipMemcpyAsync(ctx->fo_vis.p, visible, nq * 4, hipMemcpyHostToDevice, st));
    if (int rc = found_index(ctx, (const sdf_search_found *)ctx->fo_found.p, nf, (size_t)entries, nullptr, (const uint32_t *)ctx->fo_vis.p, st, &F))
      return rc;
    Fp = &F;
  }
  SDF_HIP(ctx->sw_q.reserve(nq * sizeof(sdf_minimizer)));
  SDF_HIP(ctx->sw_r.reserve(nr * sizeof(sdf_minimizer)));
  SDF_HIP(ctx->sw_limit.reserve(n_limit * 4));
  SDF_HIP(ctx->sw_first.reserve((nq + 1) * 8));
  SDF_HIP(ctx->sw_win.reserve(nq * sizeof(sdf_search_window)));
  const sdf_minimizer *d_q = (const sdf_minimizer *)ctx->sw_q.p, *d_r = (const sdf_minimizer *)ctx->sw_r.p;
  const int32_t *d_limit = (const int32_t *)ctx->sw_limit.p;
  uint64_t *d_first = (uint64_t *)ctx->sw_first.p;
  SDF_HIP(hipMemcpyAsync(ctx->sw_q.p, q, nq * sizeof(sdf_minimizer), hipMemcpyHostToDevice, st));
  if (nr) SDF_HIP(hipMemcpyAsync(ctx->sw_r.p, r_sorted, nr * sizeof(sdf_minimizer), hipMemcpyHostToDevice, st));
  if (n_limit) SDF_HIP(hipMemcpyAsync(ctx->sw_limit.p, limit, n_limit * 4, hipMemcpyHostToDevice, st));
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
struct RollArgs {
  const sdf_minimizer *q;
  size_t nq;
  const sdf_search_window *windows;
  const uint64_t *first;
  const sdf_search_interval *intervals;
  const sdf_minimizer *r;
  size_t nr;
  int64_t len_r;
  int32_t init_len;
  const int32_t *limit;
  size_t n_limit;
};

// what every form checks of its scalars (n: the intervals, or the wavefronts of the device form)
int roll_scalars(size_t nq, size_t n, size_t nr, int64_t len_r, int32_t init_len, size_t n_limit, const char **why) {
  if (init_len < 1) return *why = "search roll: init_len < 1", SDF_ERR_INVALID;
  if (len_r < 0) return *why = "search roll: len_r < 0", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search roll implements init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x3fffffffu) return *why = "search roll: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (nr > 0x7fffffffu || n_limit > 0x7fffffffu || n > 0x7fffffffu || len_r > 0x7fffffff)
    return *why = "search roll: more than 2^31 - 1 reference records, limit entries, intervals or bases in one call", SDF_ERR_UNSUPPORTED;
  if (n > 0 && nr == 0) return *why = "search roll: intervals without a reference record", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and the host forms of their arrays
int roll_arrays(const RollArgs &A, const void *out, const char **why) {
  if (!A.q || !A.windows || !A.first) return *why = "search roll: invalid arguments", SDF_ERR_INVALID;
  if (A.first[0] != 0) return *why = "search roll: first[0] != 0", SDF_ERR_INVALID;
  for (size_t i = 0; i < A.nq; i++)
    if (A.first[i + 1] < A.first[i]) return *why = "search roll: first[] does not ascend", SDF_ERR_INVALID;
  const uint64_t n = A.first[A.nq];
  if (n > 0x7fffffffu) return roll_scalars(A.nq, (size_t)0x80000000u, A.nr, A.len_r, A.init_len, A.n_limit, why);
  if (int rc = roll_scalars(A.nq, (size_t)n, A.nr, A.len_r, A.init_len, A.n_limit, why)) return rc;
  if (n && (!A.intervals || !out || !A.r || !A.limit)) return *why = "search roll: invalid arguments", SDF_ERR_INVALID;
  for (size_t i = 0; i < A.nq; i++) {
    if (A.first[i + 1] == A.first[i]) continue;
    const sdf_search_window &W = A.windows[i];
    if (W.query_size < 0 || (size_t)W.query_size >= A.n_limit)
      return *why = "search roll: a window with intervals has a query_size outside the limit table", SDF_ERR_INVALID;
    if (W.n_members < 1 || (size_t)W.n_members > A.nq - i)
      return *why = "search roll: a window with intervals has n_members outside 1 .. nq - i", SDF_ERR_INVALID;
    for (uint64_t t = A.first[i]; t < A.first[i + 1]; t++)
      if (A.intervals[t].start < 0 || A.intervals[t].start > A.intervals[t].end)
        return *why = "search roll: an interval with start < 0 or start > end", SDF_ERR_INVALID;
  }
  return SDF_OK;
}

// The walk of include/sedef_hip.h (steps 1 to 5) for interval T, from event to event; span0: the first record with
// loc >= T.start.  eval(s, e, ws, we) at every evaluation of J -- step 4 and every round with an event --; true ends the walk.
template <class Add, class Remove, class Eval>
void roll_walk(const RollArgs &A, const sdf_search_interval &T, size_t span0, Add add, Remove remove, Eval eval) {
  const sdf_minimizer *r = A.r;
  const int64_t len_r = A.len_r, init_len = A.init_len;
  int64_t s = T.start, e = std::min(s + init_len, len_r);
  size_t ws = span0, we = span0;
  while (we < A.nr && (int64_t)r[we].loc < e) add(r[we++]);
  if (eval(s, e, ws, we)) return;
  while (s < T.end && e < len_r) {  // (e was not clamped: e == s + init_len)
    // the next step with an event: a remove at the first s' >= s with loc <= s', an add at loc == s' + init_len
    int64_t next = -1;
    if (ws < A.nr) next = std::max<int64_t>(r[ws].loc, s);
    if (we < A.nr && (int64_t)r[we].loc >= e) {
      const int64_t at = (int64_t)r[we].loc - init_len;
      next = next < 0 || at < next ? at : next;
    }
    if (next < 0 || next >= T.end || next + init_len >= len_r) break;
    s = next, e = next + init_len;
    if (ws < A.nr && (int64_t)r[ws].loc <= s) remove(r[ws++]);
    if (we < A.nr && (int64_t)r[we].loc == e) add(r[we++]);
    if (eval(s, e, ws, we)) return;
    s++, e++;
  }
}

// Interval T of window i as include/sedef_hip.h states it: a map in place of the reference's, the walk from event to event.
// (Of A it reads windows[i] alone and never first[]: sdf::pair_host_window passes one window's intervals with first == nullptr;
// extend_one likewise, with intervals[] and rolls[] indexed from the window's first interval.)
void roll_one(const RollArgs &A, size_t i, const sdf_search_interval &T, sdf_search_roll_rec &R, std::map<uint64_t, uint8_t> &M) {
  const sdf_search_window &W = A.windows[i];
  const auto loc_less = [](const sdf_minimizer &m, int64_t loc) { return (int64_t)m.loc < loc; };
  const auto less_loc = [](int64_t loc, const sdf_minimizer &m) { return loc < (int64_t)m.loc; };
  const sdf_minimizer *r = A.r, *r_end = A.r + A.nr;
  const size_t span0 = (size_t)(std::lower_bound(r, r_end, (int64_t)T.start, loc_less) - r);
  const size_t span1 = (size_t)(std::upper_bound(r + span0, r_end, (int64_t)T.end + A.init_len, less_loc) - r);
  R.flags = W.n_members > SDF_SEARCH_MAX_MEMBERS || span1 - span0 > SDF_ROLL_MAX_SPAN ? SDF_ROLL_WIDE : 0;
  M.clear();
  for (int32_t j = 0; j < W.n_members; j++) M[search_host_key(A.q[i + j])] = 1;
  auto B = std::prev(M.end());
  int64_t I = 0;
  const int64_t L = A.limit[W.query_size];
  const auto add = [&](const sdf_minimizer &m) {
    if (m.status == 2) return;
    const uint64_t k = search_host_key(m);
    auto it = M.lower_bound(k);
    if (it != M.end() && it->first == k) {
      if (it->second & 2) return;
      it->second = 3;
      I += k < B->first;
      return;
    }
    M.insert(it, {k, (uint8_t)2});
    if (k < B->first) {
      I -= B->second == 3;
      --B;
    }
  };
  const auto remove = [&](const sdf_minimizer &m) {
    if (m.status == 2) return;
    const uint64_t k = search_host_key(m);
    auto it = M.find(k);
    if (it == M.end() || !(it->second & 2)) return;
    if (k <= B->first) {
      I -= it->second == 3;
      if (it->second == 2 && std::next(B) != M.end()) {
        ++B;
        I += B->second == 3;
      }
    }
    if (it->second == 2) M.erase(it);
    else it->second = 1;
  };
  const auto J = [&]() { return (int32_t)(I >= L ? I : I - L); };
  bool any = false;
  roll_walk(A, T, span0, add, remove, [&](int64_t s, int64_t e, size_t ws, size_t we) {
    if (!any || J() > R.jaccard)
      R.ref_start = (int32_t)s, R.ref_end = (int32_t)e, R.winnow_start = (int32_t)ws, R.winnow_end = (int32_t)we, R.jaccard = J();
    any = true;
    return false;
  });
}

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

extern "C" int sdf_search_roll_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                    const sdf_search_interval *intervals, const sdf_minimizer *r, size_t nr, int64_t len_r, int32_t init_len,
                                    const int32_t *limit, size_t n_limit, sdf_search_roll_rec *out) {
  if (nq == 0) return SDF_OK;
  const RollArgs A{q, nq, windows, first, intervals, r, nr, len_r, init_len, limit, n_limit};
  const char *why = nullptr;
  if (int rc = roll_arrays(A, out, &why)) return rc;
  std::map<uint64_t, uint8_t> M;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++) roll_one(A, i, intervals[t], out[t], M);
  return SDF_OK;
}

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
  struct Copy {
    DevBuf &buf;
    const void *src;
    size_t bytes;
  } copies[] = {{ctx->sr_q, q, nq * sizeof(sdf_minimizer)},  {ctx->sr_win, windows, nq * sizeof(sdf_search_window)},
                {ctx->sr_first, first, (nq + 1) * 8},        {ctx->sr_iv, intervals, n * sizeof(sdf_search_interval)},
                {ctx->sr_r, r, nr * sizeof(sdf_minimizer)},  {ctx->sr_limit, limit, n_limit * 4}};
  for (Copy &c : copies) {
    SDF_HIP(c.buf.reserve(c.bytes));
    SDF_HIP(hipMemcpyAsync(c.buf.p, c.src, c.bytes, hipMemcpyHostToDevice, st));
  }
  SDF_HIP(ctx->sr_out.reserve(n * sizeof(sdf_search_roll_rec)));
  if (int rc = roll_launch<true>(ctx, (const sdf_minimizer *)ctx->sr_q.p, nq, (const sdf_search_window *)ctx->sr_win.p,
                                 (const uint64_t *)ctx->sr_first.p, (const sdf_search_interval *)ctx->sr_iv.p, n,
                                 (const sdf_minimizer *)ctx->sr_r.p, nr, len_r, init_len, (const int32_t *)ctx->sr_limit.p, n_limit,
                                 (sdf_search_roll_rec *)ctx->sr_out.p, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->sr_out.p, n * sizeof(sdf_search_roll_rec), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  // the WIDE intervals, on the host
  std::map<uint64_t, uint8_t> M;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++)
      if (out[t].flags & SDF_ROLL_WIDE) roll_one(A, i, intervals[t], out[t], M);
  return SDF_OK;
}

// ---- the extension ----

namespace {
struct ExtendArgs {
  RollArgs R;
  const sdf_search_roll_rec *rolls;
  const sdf_filter_rec *filter;  // or null
  int64_t len_q;
  sdf_extend_params P;
};

int extend_scalars(int64_t len_q, const sdf_extend_params *P, const char **why) {
  if (!P) return *why = "search extend: invalid arguments", SDF_ERR_INVALID;
  if (len_q < 0) return *why = "search extend: len_q < 0", SDF_ERR_INVALID;
  if (!std::isfinite(P->max_error) || !std::isfinite(P->max_edit_error)) return *why = "search extend: a parameter that is not finite", SDF_ERR_INVALID;
  if (!(P->max_error - P->max_edit_error > 0)) return *why = "search extend: max_error - max_edit_error <= 0", SDF_ERR_INVALID;
  if (len_q > 0x7fffffff) return *why = "search extend: more than 2^31 - 1 query bases", SDF_ERR_UNSUPPORTED;
  if (P->reserved[0] || P->reserved[1]) return *why = "search extend: reserved != 0", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

// The SlidingMap of include/sedef_hip.h: bits by key (a key is stored while its bits are not 0), the boundary key B or none, I.
struct ExtendMap {
  std::map<uint64_t, uint8_t> M;
  bool has_B = false;
  uint64_t B = 0;
  int64_t I = 0;
  bool full(uint64_t k) const {
    const auto it = M.find(k);
    return it != M.end() && it->second == 3;
  }
  void to_below() {  // B = the largest stored key below B, or none
    auto it = M.lower_bound(B);
    if (it == M.begin()) has_B = false;
    else B = std::prev(it)->first;
  }
  bool to_above() {  // B = the smallest stored key above B; false, and B stays: there is none
    const auto it = M.upper_bound(B);
    if (it == M.end()) return false;
    B = it->first;
    return true;
  }
  bool add(uint64_t k, uint8_t BIT, bool counted) {
    uint8_t &b = M[k];
    if (b & BIT) return false;
    const uint8_t was = b;
    b |= BIT;
    if (counted && has_B && k < B) {
      I += b == 3;
      if (was == 0) {
        I -= full(B);
        to_below();
      }
    }
    return true;
  }
  bool remove(uint64_t k, uint8_t BIT, bool counted) {
    const auto it = M.find(k);
    if (it == M.end() || !(it->second & BIT)) return false;
    if (counted && has_B && k <= B) {
      I -= it->second == 3;
      if (it->second == BIT && to_above()) I += full(B);
    }
    if (it->second == BIT) M.erase(it);
    else it->second &= (uint8_t)~BIT;
    return true;
  }
};

// Interval t of window i as include/sedef_hip.h states it: the entry state by the roll's walk, then the extension.
void extend_one(const ExtendArgs &A, size_t i, uint64_t t, sdf_search_hit &H, ExtendMap &S) {
  const RollArgs &RA = A.R;
  const sdf_search_window &W = RA.windows[i];
  const sdf_search_interval &T = RA.intervals[t];
  const sdf_search_roll_rec &Roll = A.rolls[t];
  const sdf_minimizer *q = RA.q, *r = RA.r;
  const int64_t nq = (int64_t)RA.nq, nr = (int64_t)RA.nr;
  H = sdf_search_hit{0, 0, 0, 0, 0, 0, 0, 0, 0, 0u};
  const int64_t lo = std::lower_bound(r, r + nr, (int64_t)T.start, [](const sdf_minimizer &m, int64_t loc) { return (int64_t)m.loc < loc; }) - r;
  if (extend_skips(Roll, A.filter ? &A.filter[t] : nullptr, lo, nr)) {
    H.flags = SDF_EXTEND_SKIPPED;
    return;
  }
  bool wide = extend_replay_wide(Roll, W.n_members, lo), nolimit = false;
  // the entry state
  S.M.clear();
  for (int32_t j = 0; j < W.n_members; j++) S.M[search_host_key(q[i + j])] = 1;
  S.has_B = true, S.B = std::prev(S.M.end())->first, S.I = 0;
  const int64_t rws0 = Roll.winnow_start, rwe0 = Roll.winnow_end;
  roll_walk(
      RA, T, (size_t)lo, [&](const sdf_minimizer &m) { m.status == 2 ? false : S.add(search_host_key(m), 2, true); },
      [&](const sdf_minimizer &m) { m.status == 2 ? false : S.remove(search_host_key(m), 2, true); },
      [&](int64_t, int64_t, size_t ws, size_t we) { return (int64_t)ws >= rws0 && (int64_t)we >= rwe0; });
  int64_t qsz = W.query_size, L = RA.limit[qsz];
  int64_t qws = (int64_t)i, qwe = (int64_t)i + W.n_members, rws = rws0, rwe = rwe0;
  const int64_t qws0 = qws, qwe0 = qwe;
  const auto add_to_query = [&](const sdf_minimizer &m) {
    if (!S.add(search_host_key(m), 1, qsz != 0)) return;
    if (++qsz >= (int64_t)RA.n_limit) {
      nolimit = true;
      return;
    }
    L = RA.limit[qsz];
    if (!S.has_B) S.has_B = true, S.B = S.M.begin()->first;
    else S.to_above();
    S.I += S.full(S.B);
  };
  const auto remove_from_query = [&](const sdf_minimizer &m) {
    if (!S.remove(search_host_key(m), 1, qsz != 0)) return;
    if (qsz > 0) --qsz;
    L = RA.limit[qsz];
    if (!S.has_B) return;
    S.I -= S.full(S.B);
    S.to_below();
  };
  const auto add_to_reference = [&](const sdf_minimizer &m) {
    if (m.status != 2) S.add(search_host_key(m), 2, qsz != 0);
  };
  const auto remove_from_reference = [&](const sdf_minimizer &m) {
    if (m.status != 2) S.remove(search_host_key(m), 2, qsz != 0);
  };
  const auto J = [&]() { return (int32_t)(S.I >= L ? S.I : S.I - L); };
  int32_t qs = qws ? q[qws - 1].loc + 1 : 0, qe = qwe < nq ? (int32_t)q[qwe].loc : (int32_t)A.len_q;
  int32_t rs = rws ? r[rws - 1].loc + 1 : 0, re = rwe < nr ? (int32_t)r[rwe].loc : (int32_t)RA.len_r;
  while (!nolimit && !extend_stops(A.P, qs, qe, rs, re)) {
    bool extended = false;
    for (int way = 0; way < 3 && !extended && !nolimit; way++) {  // both_both, both_right, both_left
      const bool left = way != 1, right = way != 2;
      if (left && (!qws || !rws)) continue;
      if (right && (rwe >= nr || qwe >= nq)) continue;
      // the growth cap, for every side of the step before its first add (the kernel ends here)
      wide |= left && (qws0 - qws >= SDF_EXTEND_MAX_GROW || rws0 - rws >= SDF_EXTEND_MAX_GROW);
      wide |= right && (qwe - qwe0 >= SDF_EXTEND_MAX_GROW || rwe - rwe0 >= SDF_EXTEND_MAX_GROW);
      if (left) {
        add_to_query(q[--qws]), qs = qws ? q[qws - 1].loc + 1 : 0;
        add_to_reference(r[--rws]), rs = rws ? r[rws - 1].loc + 1 : 0;
      }
      if (right && !nolimit) {
        add_to_query(q[qwe++]), qe = qwe < nq ? (int32_t)q[qwe].loc : (int32_t)A.len_q;
        add_to_reference(r[rwe++]), re = rwe < nr ? (int32_t)r[rwe].loc : (int32_t)RA.len_r;
      }
      if (nolimit) break;
      if (J() >= 0) {
        extended = true;
        break;
      }
      if (right) {  // the reference's undo: removes in its order, not a restore
        remove_from_reference(r[--rwe]), re = (int32_t)r[rwe].loc;
        remove_from_query(q[--qwe]), qe = (int32_t)q[qwe].loc;
      }
      if (left) {
        rs = (int32_t)r[rws].loc + 1, remove_from_reference(r[rws++]);
        qs = (int32_t)q[qws].loc + 1, remove_from_query(q[qws++]);
      }
    }
    if (!extended) break;
  }
  if (nolimit) {
    H.flags = SDF_EXTEND_NOLIMIT | (wide ? (uint32_t)SDF_EXTEND_WIDE : 0u);
    return;
  }
  H = sdf_search_hit{qs, qe, rs, re, J(), (int32_t)qws, (int32_t)qwe, (int32_t)rws, (int32_t)rwe, wide ? (uint32_t)SDF_EXTEND_WIDE : 0u};
}

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

extern "C" int sdf_search_extend_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                      const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, const sdf_filter_rec *filter,
                                      const sdf_minimizer *r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *limit,
                                      size_t n_limit, const sdf_extend_params *params, sdf_search_hit *out) {
  if (nq == 0) return SDF_OK;
  const RollArgs RA{q, nq, windows, first, intervals, r, nr, len_r, init_len, limit, n_limit};
  const char *why = nullptr;
  if (int rc = roll_arrays(RA, out, &why)) return rc;
  if (first[nq] == 0) return SDF_OK;
  if (!rolls) return SDF_ERR_INVALID;
  if (int rc = extend_scalars(len_q, params, &why)) return rc;
  const ExtendArgs A{RA, rolls, filter, len_q, *params};
  ExtendMap S;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++) extend_one(A, i, t, out[t], S);
  return SDF_OK;
}

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

// The workspace of a call and the launches that fill it.  Everything here follows from n_max, n_long_max, long_grow and batch.
struct ExtendLongPlan {
  size_t batch, stride, items, batches;
  size_t off_flag, off_pos, off_list, off_meta, off_nds, off_keys, off_keys2, off_vals, off_vals2, off_incl, off_slots, bytes, tmp_bytes;
  int end_bit;
};
int extend_long_plan(sdf_ctx *ctx, size_t n_max, size_t n_long_max, int32_t long_grow, size_t batch, ExtendLongPlan &L, hipStream_t st) {
  L.batch = std::min(std::min(batch ? batch : kExtendLongBatch, kExtendLongMaxBatch), n_long_max);
  L.stride = (size_t)SDF_SEARCH_MAX_MEMBERS + SDF_ROLL_MAX_SPAN + 4 * (size_t)long_grow;
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

// the launches, on `st`; d_left or null
int extend_long_run(sdf_ctx *ctx, const ExtLongArgs &A, size_t n_max, size_t n_long_max, size_t batch, int64_t len_q, int64_t len_r,
                    int32_t init_len, const int32_t *d_limit, const sdf_extend_params &P, sdf_search_hit *d_hits, uint64_t *d_left, hipStream_t st) {
  ExtendLongPlan L;
  if (int rc = extend_long_plan(ctx, n_max, n_long_max, A.grow, batch, L, st)) return rc;
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
  const ExtLongArgs A{d_q, d_r, d_windows, d_first, d_intervals, d_rolls, d_filter, (int)nq, (int)nr, (int)n_limit, (int)long_grow,
                      SDF_SEARCH_MAX_MEMBERS + SDF_ROLL_MAX_SPAN + 4 * (int)long_grow};
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
  struct Copy {
    DevBuf &buf;
    const void *src;
    size_t bytes;
  } copies[] = {{ctx->sr_q, q, nq * sizeof(sdf_minimizer)},          {ctx->sr_win, windows, nq * sizeof(sdf_search_window)},
                {ctx->sr_first, first, (nq + 1) * 8},                {ctx->sr_iv, intervals, n * sizeof(sdf_search_interval)},
                {ctx->sr_r, r, nr * sizeof(sdf_minimizer)},          {ctx->sr_limit, limit, n_limit * 4},
                {ctx->se_rolls, rolls, n * sizeof(sdf_search_roll_rec)}, {ctx->se_filter, filter, filter ? n * sizeof(sdf_filter_rec) : 0}};
  for (Copy &c : copies) {
    if (!c.bytes) continue;
    SDF_HIP(c.buf.reserve(c.bytes));
    SDF_HIP(hipMemcpyAsync(c.buf.p, c.src, c.bytes, hipMemcpyHostToDevice, st));
  }
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
      const int64_t lo = std::lower_bound(r, r + nr, (int64_t)intervals[t].start, [](const sdf_minimizer &m, int64_t loc) { return (int64_t)m.loc < loc; }) - r;
      n_long += !extend_replay_wide(rolls[t], windows[i].n_members, lo);
    }
  if (n_long) {
    const ExtLongArgs LA{(const sdf_minimizer *)ctx->sr_q.p, (const sdf_minimizer *)ctx->sr_r.p, (const sdf_search_window *)ctx->sr_win.p,
                         (const uint64_t *)ctx->sr_first.p, (const sdf_search_interval *)ctx->sr_iv.p, (const sdf_search_roll_rec *)ctx->se_rolls.p,
                         filter ? (const sdf_filter_rec *)ctx->se_filter.p : nullptr, (int)nq, (int)nr, (int)n_limit, SDF_EXTEND_LONG_MAX_GROW,
                         SDF_SEARCH_MAX_MEMBERS + SDF_ROLL_MAX_SPAN + 4 * SDF_EXTEND_LONG_MAX_GROW};
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

// ---- one window of initial_search, for sdf_search_pair_host (sdf_entry.h) ----

int sdf::pair_host_window(const PairHostArgs &A, size_t i, std::vector<sdf_search_found> &found, PairHostWindow &W) {
  constexpr uint32_t fail = SDF_FILTER_UPPER_FAIL | SDF_FILTER_QGRAM_FAIL | SDF_FILTER_SKIPPED;
  W.reported.clear(), W.hits.clear();
  W.attempted = W.jaccard_failed = W.interval_failed = 0;
  if (W.windows.size() < A.nq) W.windows.resize(A.nq);
  const int32_t init_len = A.min_read_size;
  const SearchArgs SA{A.q, A.nq, A.len_q, A.r_sorted, A.nr, A.r_threshold, init_len, A.same_genome, A.uppercase_seeds, A.limit, A.n_limit};
  sdf_search_window &win = W.windows[i];
  std::vector<sdf_search_interval> T;
  SearchScratch S;
  const FoundView V{found.data(), found.size()};
  search_one_window(SA, i, win, T, S, &V);
  if (T.empty()) return SDF_OK;
  const RollArgs RA{A.q, A.nq, W.windows.data(), nullptr, T.data(), A.r, A.nr, A.len_r, init_len, A.limit, A.n_limit};
  std::vector<sdf_search_roll_rec> rolls(T.size(), sdf_search_roll_rec{0, 0, 0, 0, 0, 0});
  const ExtendArgs EA{RA, rolls.data(), nullptr, A.len_q, A.extend};
  const FilterTaskArgs FA{A.len_q, A.len_r, A.q_off, A.r_off, init_len, A.q_rc, A.r_rc, 1};
  std::map<uint64_t, uint8_t> M;
  ExtendMap ES;
  const long long pf_pos = A.q[i].loc, pf_end = pf_pos + init_len;
  for (size_t t = 0; t < T.size(); t++) {
    W.attempted += 1;
    roll_one(RA, i, T[t], rolls[t], M);
    if (rolls[t].jaccard < 0) {
      W.jaccard_failed += 1;
      continue;
    }
    bool overlapped = false;
    for (size_t f = 0; f < found.size() && !overlapped; f++)
      overlapped = !found_empty(found[f]) && found_covers(found[f], pf_pos, rolls[t].ref_start) &&
                   found_overlaps(found[f], pf_pos, pf_end, rolls[t].ref_start, rolls[t].ref_end, A.min_read_size);
    if (overlapped) {
      W.interval_failed += 1;
      continue;
    }
    const sdf_filter_task task = filter_task_of(FA, pf_pos, win, T[t], rolls[t]);
    sdf_filter_rec rec;
    if (int rc = sdf_search_filter_host(A.pool, A.pool_bytes, &A.filter, &task, 1, &rec)) return rc;
    if (rec.flags & fail) continue;
    sdf_search_hit H;
    extend_one(EA, i, t, H, ES);  // (a WIDE record is completed here, and is a hit)
    if (H.flags & (SDF_EXTEND_SKIPPED | SDF_EXTEND_NOLIMIT)) continue;
    const sdf_filter_task htask = hit_task_of(FA, H);
    if (int rc = sdf_search_filter_host(A.pool, A.pool_bytes, &A.filter, &htask, 1, &rec)) return rc;
    if (rec.flags & fail) continue;
    W.hits.push_back(sdf_search_pair_hit{(int32_t)i, H.query_start, H.query_end, H.ref_start, H.ref_end, H.jaccard});
    found.push_back(sdf_search_found{H.query_start, H.query_end, H.ref_start, H.ref_end});
  }
  const auto rec_of = [](const sdf_search_pair_hit &h) { return sdf_search_found{h.query_start, h.query_end, h.ref_start, h.ref_end}; };
  for (size_t h = 0; h < W.hits.size(); h++) {  // parse_hits
    bool dropped = false;
    for (size_t p = 0; p < W.hits.size() && !dropped; p++) dropped = p != h && accept_contains(rec_of(W.hits[p]), rec_of(W.hits[h]));
    if (!dropped) W.reported.push_back(W.hits[h]);
  }
  return SDF_OK;
}
