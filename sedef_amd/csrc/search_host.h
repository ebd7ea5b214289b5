// The search family on the host (search_host.hip): the rules of include/sedef_hip.h in plain C++, item by item, and -- inline -- the checks
// that the host forms share with the device and uploading forms (sdf_search_api.hip, sdf_filter_api.hip, sdf_found_api.hip,
// sdf_driver_api.hip).  Nothing here needs a context or a stream.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "sdf_kernels.h"

namespace sdf {
// ---- the windows ----
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
// what every form checks of its scalars; *why: the refusal's text
inline int search_scalars(size_t nq, size_t nr, int32_t init_len, size_t n_limit, const char **why) {
  if (init_len < 1) return *why = "search windows: init_len < 1", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search windows implement init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x3fffffffu) return *why = "search windows: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (nr > 0x7fffffffu || n_limit > 0x7fffffffu)
    return *why = "search windows: more than 2^31 - 1 reference records or limit entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the forms that take host arrays of those
inline int search_arrays(const SearchArgs &A, const uint64_t *first, const sdf_search_window *windows, const void *out, size_t cap,
                         const size_t *used, const char **why) {
  if (!A.q || !first || !windows || !used || (cap && !out) || (A.nr && !A.r) || (A.n_limit && !A.limit))
    return *why = "search windows: invalid arguments", SDF_ERR_INVALID;
  if (int rc = search_scalars(A.nq, A.nr, A.init_len, A.n_limit, why)) return rc;
  for (size_t s = 1; s < A.n_limit; s++)
    if (A.limit[s] < 1) return *why = "search windows: a limit below 1 (the reference reads candidates[-1] there)", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... of a list of found records and its prefixes (n of them, each at most nf); *entries: the bin entries of the list
inline int found_arrays(const sdf_search_found *found, size_t nf, const uint32_t *visible, size_t n, uint64_t *entries, const char **why) {
  if ((nf && !found) || (n && !visible)) return *why = "search found: invalid arguments", SDF_ERR_INVALID;
  if (nf > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 found records in one call", SDF_ERR_UNSUPPORTED;
  for (size_t t = 0; t < n; t++)
    if (visible[t] > nf) return *why = "search found: a prefix longer than the list", SDF_ERR_INVALID;
  sdf_search_found_entries(found, nf, entries);
  if (*entries > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 bin entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// Window i as include/sedef_hip.h states it, step by step: its record, its intervals appended to T.  F: the found records the
// window sees, a linear pass per gathered position (null: an empty tree).
void search_one_window(const SearchArgs &A, size_t i, sdf_search_window &W, std::vector<sdf_search_interval> &T, SearchScratch &S,
                       const FoundView *F);

// ---- the roll and the extension ----
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
struct ExtendArgs {
  RollArgs R;
  const sdf_search_roll_rec *rolls;
  const sdf_filter_rec *filter;  // or null
  int64_t len_q;
  sdf_extend_params P;
};
// The SlidingMap of include/sedef_hip.h, the one map of the roll and the extension: bits by key (a key is stored while its
// bits are not 0), the boundary key B or none, I.  `at`: the first stored key at or after B (M.end(): none), kept through
// every change, so that B moves without a descent of the map.
struct ExtendMap {
  using Map = std::map<uint64_t, uint8_t>;
  Map M;
  Map::iterator at;
  bool has_B = false;
  uint64_t B = 0;
  int64_t I = 0;
  // the entry state of an interval's walk: the window's n members at 1, B the largest key, I = 0
  void enter(const sdf_minimizer *members, int32_t n);
  bool B_full() const { return at != M.end() && at->first == B && at->second == 3; }  // B is stored with both bits
  void to_first() { has_B = true, at = M.begin(), B = at->first; }  // B = the smallest stored key
  bool to_below() {  // B = the largest stored key below B, or none; true: the key that B leaves was full
    const bool was_full = B_full();
    if (at == M.begin()) has_B = false;
    else B = (--at)->first;
    return was_full;
  }
  int to_above() {  // B = the smallest stored key above B: 1 when that key is full, else 0; -1, and B stays: there is none
    const auto it = at != M.end() && at->first == B ? std::next(at) : at;
    if (it == M.end()) return -1;
    at = it, B = it->first;
    return it->second == 3;
  }
  bool add(uint64_t k, uint8_t BIT, bool counted) {
    auto it = M.lower_bound(k);
    if (it == M.end() || it->first != k) {
      it = M.emplace_hint(it, k, (uint8_t)0);
      if (k >= B && (at == M.end() || k < at->first)) at = it;
    }
    uint8_t &b = it->second;
    if (b & BIT) return false;
    const uint8_t was = b;
    b |= BIT;
    if (counted && has_B && k < B) {
      I += b == 3;
      if (was == 0) I -= to_below();
    }
    return true;
  }
  bool remove(uint64_t k, uint8_t BIT, bool counted) {
    const auto it = M.find(k);
    if (it == M.end() || !(it->second & BIT)) return false;
    if (counted && has_B && k <= B) {
      I -= it->second == 3;
      if (it->second == BIT) I += to_above() > 0;
    }
    if (it->second != BIT) it->second &= (uint8_t)~BIT;
    else if (it == at) at = M.erase(it);
    else M.erase(it);
    return true;
  }
};
// what every form checks of its scalars (n: the intervals, or the wavefronts of the device form)
inline int roll_scalars(size_t nq, size_t n, size_t nr, int64_t len_r, int32_t init_len, size_t n_limit, const char **why) {
  if (init_len < 1) return *why = "search roll: init_len < 1", SDF_ERR_INVALID;
  if (len_r < 0) return *why = "search roll: len_r < 0", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search roll implements init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x3fffffffu) return *why = "search roll: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (nr > 0x7fffffffu || n_limit > 0x7fffffffu || n > 0x7fffffffu || len_r > 0x7fffffff)
    return *why = "search roll: more than 2^31 - 1 reference records, limit entries, intervals or bases in one call", SDF_ERR_UNSUPPORTED;
  if (n > 0 && nr == 0) return *why = "search roll: intervals without a reference record", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and the forms that take host arrays of those
inline int roll_arrays(const RollArgs &A, const void *out, const char **why) {
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
inline int extend_scalars(int64_t len_q, const sdf_extend_params *P, const char **why) {
  if (!P) return *why = "search extend: invalid arguments", SDF_ERR_INVALID;
  if (len_q < 0) return *why = "search extend: len_q < 0", SDF_ERR_INVALID;
  if (!std::isfinite(P->max_error) || !std::isfinite(P->max_edit_error)) return *why = "search extend: a parameter that is not finite", SDF_ERR_INVALID;
  if (!(P->max_error - P->max_edit_error > 0)) return *why = "search extend: max_error - max_edit_error <= 0", SDF_ERR_INVALID;
  if (len_q > 0x7fffffff) return *why = "search extend: more than 2^31 - 1 query bases", SDF_ERR_UNSUPPORTED;
  if (P->reserved[0] || P->reserved[1]) return *why = "search extend: reserved != 0", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// the first record of r[0, nr), ascending loc, with loc at or after `loc`
inline size_t first_at_or_after(const sdf_minimizer *r, size_t nr, int64_t loc) {
  return (size_t)(std::lower_bound(r, r + nr, loc, [](const sdf_minimizer &m, int64_t at) { return (int64_t)m.loc < at; }) - r);
}
// Interval T of window i as include/sedef_hip.h states it, the walk from event to event.  (Of A it reads windows[i] alone and
// never first[]: pair_host_window passes one window's intervals with first == nullptr; extend_one likewise, with intervals[]
// and rolls[] indexed from the window's first interval.)
void roll_one(const RollArgs &A, size_t i, const sdf_search_interval &T, sdf_search_roll_rec &R, ExtendMap &S);
// Interval t of window i as include/sedef_hip.h states it: the entry state by the roll's walk, then the extension.
void extend_one(const ExtendArgs &A, size_t i, uint64_t t, sdf_search_hit &H, ExtendMap &S);

// ---- the filter and its tasks ----
// what every form checks of its parameters and n
inline int filter_scalars(const sdf_filter_params *P, size_t n, const char **why) {
  if (!P) return *why = "search filter: invalid arguments", SDF_ERR_INVALID;
  if (!std::isfinite(P->max_error) || !std::isfinite(P->max_edit_error) || !std::isfinite(P->gap_frequency))
    return *why = "search filter: a parameter that is not finite", SDF_ERR_INVALID;
  if (P->reserved != 0) return *why = "search filter: reserved != 0 in the parameters", SDF_ERR_UNSUPPORTED;
  if (n > 0x7fffffffu) return *why = "search filter: more than 2^31 - 1 tasks in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the forms that take host arrays of their tasks, in order; the first refusal is the call's
inline int filter_tasks(const sdf_filter_task *tasks, size_t n, size_t pool_bytes, bool *any_rc, bool *any_long, std::string *why) {
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
// what every form of the task builders checks of its scalars (n: the intervals or hits, or the lanes of the device form)
inline int filter_tasks_scalars(size_t nq, size_t n, int64_t len_q, int64_t len_r, int32_t init_len, int64_t q_off, int64_t r_off, const char **why) {
  if (init_len < 1) return *why = "search filter tasks: init_len < 1", SDF_ERR_INVALID;
  if (len_q < 0 || len_r < 0 || q_off < 0 || r_off < 0) return *why = "search filter tasks: a negative length or offset", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search filter tasks implement init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x7fffffffu || n > 0x7fffffffu || len_q > 0x7fffffff || len_r > 0x7fffffff)
    return *why = "search filter tasks: more than 2^31 - 1 query minimizers, intervals or bases in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
inline int hit_tasks_scalars(size_t n, int64_t len_q, int64_t len_r, int64_t q_off, int64_t r_off, const char **why) {
  if (len_q < 0 || len_r < 0 || q_off < 0 || r_off < 0) return *why = "search hit tasks: a negative length or offset", SDF_ERR_INVALID;
  if (n > 0x7fffffffu || len_q > 0x7fffffff || len_r > 0x7fffffff)
    return *why = "search hit tasks: more than 2^31 - 1 hits or bases in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

// ---- the found records: is_overlap ----
// what every form of the overlap call checks of its scalars (n: the intervals, or the lanes of the device form)
inline int overlap_scalars(size_t nq, size_t n, int32_t init_len, int32_t min_read_size, const char **why) {
  if (init_len < 1) return *why = "search overlap: init_len < 1", SDF_ERR_INVALID;
  if (min_read_size < 0) return *why = "search overlap: min_read_size < 0", SDF_ERR_INVALID;
  if (init_len > (1 << 30)) return *why = "search overlap implements init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (nq > 0x3fffffffu) return *why = "search overlap: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (n > 0x7fffffffu) return *why = "search overlap: more than 2^31 - 1 intervals in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the forms that take host arrays of those; *entries: the bin entries of the list
inline int overlap_arrays(const sdf_minimizer *q, size_t nq, const uint64_t *first, const sdf_search_roll_rec *rolls, const sdf_search_found *found,
                          size_t nf, const uint32_t *visible_iv, int32_t init_len, int32_t min_read_size, const uint32_t *out, uint64_t *entries,
                          const char **why) {
  if (!q || !first || (nf && !found)) return *why = "search overlap: invalid arguments", SDF_ERR_INVALID;
  if (first[0] != 0) return *why = "search overlap: first[0] != 0", SDF_ERR_INVALID;
  for (size_t i = 0; i < nq; i++)
    if (first[i + 1] < first[i]) return *why = "search overlap: first[] does not ascend", SDF_ERR_INVALID;
  const uint64_t n = first[nq];
  if (int rc = overlap_scalars(nq, n > 0x7fffffffu ? (size_t)0x80000000u : (size_t)n, init_len, min_read_size, why)) return rc;
  if (nf > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 found records in one call", SDF_ERR_UNSUPPORTED;
  if (n && (!rolls || !visible_iv || !out)) return *why = "search overlap: invalid arguments", SDF_ERR_INVALID;
  for (uint64_t t = 0; t < n; t++)
    if (visible_iv[t] > nf) return *why = "search found: a prefix longer than the list", SDF_ERR_INVALID;
  sdf_search_found_entries(found, nf, entries);
  if (*entries > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 bin entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

// ---- the driver ----
// what every form of the acceptance step checks of its scalars and of the pointers a count makes necessary
inline int accept_scalars(const sdf_search_accept_round *R, const void *found, size_t nf, size_t found_cap, const void *out, size_t n_out,
                          size_t out_cap, const void *status, const char **why) {
  if (!R || !status) return *why = "search accept: invalid arguments", SDF_ERR_INVALID;
  if (R->init_len < 1) return *why = "search accept: init_len < 1", SDF_ERR_INVALID;
  if (R->min_read_size < 0) return *why = "search accept: min_read_size < 0", SDF_ERR_INVALID;
  if (nf > found_cap || n_out > out_cap) return *why = "search accept: a count beyond its capacity", SDF_ERR_INVALID;
  if ((found_cap && !found) || (out_cap && !out)) return *why = "search accept: invalid arguments", SDF_ERR_INVALID;
  if (R->na && (!R->act || !R->q || !R->windows || !R->first)) return *why = "search accept: invalid arguments", SDF_ERR_INVALID;
  if (R->na && R->n_max && (!R->rolls || !R->overlap || !R->filter || !R->hits || !R->hit_filter))
    return *why = "search accept: invalid arguments", SDF_ERR_INVALID;
  if (R->init_len > (1 << 30)) return *why = "search accept implements init_len up to 2^30", SDF_ERR_UNSUPPORTED;
  if (R->nq > 0x3fffffffu) return *why = "search accept: more than 2^30 - 1 query minimizers in one call", SDF_ERR_UNSUPPORTED;
  if (R->na > 0x7fffffffu || R->n_max > 0x7fffffffu || found_cap > 0x7fffffffu || out_cap > 0x7fffffffu)
    return *why = "search accept: more than 2^31 - 1 round windows, intervals or records in one call", SDF_ERR_UNSUPPORTED;
  if (R->reserved != 0) return *why = "search accept: reserved != 0", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// ... and the forms that take host arrays of those
inline int accept_arrays(const sdf_search_accept_round *R, const char **why) {
  if (!R->na) return SDF_OK;
  for (size_t j = 0; j < R->na; j++)
    if (R->act[j] >= R->nq || (j && R->act[j] <= R->act[j - 1]))
      return *why = "search accept: act[] does not ascend strictly inside [0, nq)", SDF_ERR_INVALID;
  if (R->first[0] != 0) return *why = "search accept: first[0] != 0", SDF_ERR_INVALID;
  for (size_t i = 0; i < R->nq; i++)
    if (R->first[i + 1] < R->first[i]) return *why = "search accept: first[] does not ascend", SDF_ERR_INVALID;
  return SDF_OK;
}
inline int pair_checks(size_t pool_bytes, const sdf_minim_range *Q, const sdf_minim_range *R, const sdf_search_pair_params *P) {
  if (!Q || !R || !P || (P->n_limit && !P->limit)) return SDF_ERR_INVALID;
  for (const sdf_minim_range *r : {Q, R})
    if (!in_range(r->off, (int64_t)r->len, pool_bytes)) return SDF_ERR_INVALID;
  if (P->min_read_size < 1) return SDF_ERR_INVALID;
  if (P->same_genome && (Q->off != R->off || Q->len != R->len || Q->flags || R->flags)) return SDF_ERR_INVALID;
  const sdf_filter_params &F = P->filter;
  const sdf_extend_params &E = P->extend;
  if (!std::isfinite(F.max_error) || !std::isfinite(F.max_edit_error) || !std::isfinite(F.gap_frequency) || !std::isfinite(E.max_error) ||
      !std::isfinite(E.max_edit_error) || !(E.max_error - E.max_edit_error > 0))
    return SDF_ERR_INVALID;
  if (P->k < 1 || P->k > 15 || P->w < 1 || P->w > SDF_MINIM_MAX_W) return SDF_ERR_UNSUPPORTED;
  if ((Q->flags | R->flags) & ~SDF_MINIM_RC) return SDF_ERR_UNSUPPORTED;
  if (P->n_limit > 0x7fffffffu || P->min_read_size > (1 << 30)) return SDF_ERR_UNSUPPORTED;
  for (size_t s = 1; s < P->n_limit; s++)
    if (P->limit[s] < 1) return SDF_ERR_UNSUPPORTED;
  if (F.reserved || E.reserved[0] || E.reserved[1]) return SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}
// the schedule: no window starts in front of this base once the window at `loc` has reported hits of min_read_size or more
inline int64_t pair_next_loc(int64_t loc, int32_t min_read_size, double max_error) {
  return (int64_t)(int)((double)loc + ((double)min_read_size * max_error) / 2);
}
// the extension's parameters as a pair's stages take them
inline sdf_extend_params pair_extend_params(const sdf_search_pair_params &P) {
  sdf_extend_params E = P.extend;
  E.same_genome = P.same_genome != 0;
  return E;
}
// One window of initial_search on the host, for sdf_search_pair_host and the windows sdf_search_pair hands to the host:
// pair_host_window runs window i against the whole of `found`, appends the records it keeps to it as it goes, and leaves the
// parse_hits survivors and the counters in W.
struct PairHostArgs {
  const char *pool;
  size_t pool_bytes;
  const sdf_minimizer *q;
  size_t nq;
  const sdf_minimizer *r, *r_sorted;  // ascending loc; ascending (status, hash, loc)
  size_t nr;
  uint32_t r_threshold;
  int64_t len_q, len_r, q_off, r_off;
  int q_rc, r_rc;
  int32_t min_read_size;
  bool same_genome, uppercase_seeds;
  const int32_t *limit;
  size_t n_limit;
  sdf_filter_params filter;
  sdf_extend_params extend;
};
struct PairHostWindow {
  std::vector<sdf_search_pair_hit> reported;
  int64_t attempted = 0, jaccard_failed = 0, interval_failed = 0;
  std::vector<sdf_search_window> windows;  // scratch: nq records, of which the call fills its own
  std::vector<sdf_search_pair_hit> hits;
};
// Q, R: the ranges as they lie in `pool`; r: the reference's minimizers in ascending loc (q's own under same_genome)
PairHostArgs pair_host_args(const char *pool, size_t pool_bytes, const sdf_minim_range &Q, const sdf_minim_range &R,
                            const sdf_search_pair_params &P, const sdf_extend_params &E, const std::vector<sdf_minimizer> &q,
                            const std::vector<sdf_minimizer> &r, const std::vector<sdf_minimizer> &r_sorted, uint32_t threshold);
int pair_host_window(const PairHostArgs &A, size_t i, std::vector<sdf_search_found> &found, PairHostWindow &W);
}  // namespace sdf
