// The host statement of the search family: every rule of include/sedef_hip.h's search sections in plain C++ -- one window's
// intervals, the roll and the extension on the one sliding map, the filter, is_overlap, the acceptance step, and
// initial_search window by window with minimizers and index as tests/minim_model.py states them -- with the `_host` entry
// points over them and the checks the device and uploading forms share (search_host.h).  No context, no stream, no launch:
// the verdicts and predicates are the __host__ __device__ functions of sdf_kernels.h that the kernels use.
#include "search_host.h"

#include <cmath>
#include <cstring>
#include <deque>

#include "../../include/sedef_hip.h"

namespace {
using namespace sdf;

inline uint64_t search_host_key(const sdf_minimizer &m) { return (uint64_t)(uint32_t)m.status << 32 | m.hash; }

// rev_dna (reference: src/common.h:72-87,93) of a character below 128
inline char host_rev_dna(const char c) {
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

// is_overlap over records[0, n), a linear pass: does one of them cover (pf_pos, ref_start) and overlap the rolled interval
bool found_any_overlap(const sdf_search_found *records, size_t n, long long pf_pos, long long pf_end, long long ref_start, long long ref_end,
                       int32_t min_read_size) {
  for (size_t f = 0; f < n; f++)
    if (!found_empty(records[f]) && found_covers(records[f], pf_pos, ref_start) &&
        found_overlaps(records[f], pf_pos, pf_end, ref_start, ref_end, min_read_size))
      return true;
  return false;
}

// parse_hits over one window's kept records: dropped[h], another record of the list contains h
std::vector<uint8_t> parse_hits(const sdf_search_found *recs, size_t n) {
  std::vector<uint8_t> dropped(n, 0);
  for (size_t h = 0; h < n; h++)
    for (size_t p = 0; p < n && !dropped[h]; p++) dropped[h] = p != h && accept_contains(recs[p], recs[h]);
  return dropped;
}
}  // namespace

// ---- the windows ----

void sdf::search_one_window(const SearchArgs &A, size_t i, sdf_search_window &W, std::vector<sdf_search_interval> &T, SearchScratch &S,
                            const FoundView *F) {
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

namespace {
// sdf_search_windows_host, and with_found sdf_search_windows_found_host
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

// ---- the roll ----

void sdf::ExtendMap::enter(const sdf_minimizer *members, int32_t n) {
  M.clear();
  for (int32_t j = 0; j < n; j++) M[search_host_key(members[j])] = 1;
  has_B = true, at = std::prev(M.end()), B = at->first, I = 0;
}

namespace {
// The walk of include/sedef_hip.h (steps 1 to 5) for interval T on the map S, from event to event; span0: the first record
// with loc >= T.start.  eval(s, e, ws, we) at every evaluation of J -- step 4 and every round with an event --; true ends the walk.
template <class Eval>
void roll_walk(const RollArgs &A, const sdf_search_interval &T, size_t span0, ExtendMap &S, Eval eval) {
  const sdf_minimizer *r = A.r;
  const int64_t len_r = A.len_r, init_len = A.init_len;
  const auto add = [&](const sdf_minimizer &m) { m.status == 2 ? false : S.add(search_host_key(m), 2, true); };
  const auto remove = [&](const sdf_minimizer &m) { m.status == 2 ? false : S.remove(search_host_key(m), 2, true); };
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
}  // namespace

// (the roll is the extension's entry replay run to the end, with the best J kept)
void sdf::roll_one(const RollArgs &A, size_t i, const sdf_search_interval &T, sdf_search_roll_rec &R, ExtendMap &S) {
  const sdf_search_window &W = A.windows[i];
  const size_t span0 = first_at_or_after(A.r, A.nr, T.start);
  const size_t span1 = first_at_or_after(A.r + span0, A.nr - span0, (int64_t)T.end + A.init_len + 1) + span0;
  R.flags = W.n_members > SDF_SEARCH_MAX_MEMBERS || span1 - span0 > SDF_ROLL_MAX_SPAN ? SDF_ROLL_WIDE : 0;
  S.enter(A.q + i, W.n_members);
  const int64_t L = A.limit[W.query_size];
  bool any = false;
  roll_walk(A, T, span0, S, [&](int64_t s, int64_t e, size_t ws, size_t we) {
    const int32_t J = (int32_t)(S.I >= L ? S.I : S.I - L);
    if (!any || J > R.jaccard)
      R.ref_start = (int32_t)s, R.ref_end = (int32_t)e, R.winnow_start = (int32_t)ws, R.winnow_end = (int32_t)we, R.jaccard = J;
    any = true;
    return false;
  });
}

extern "C" int sdf_search_roll_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                    const sdf_search_interval *intervals, const sdf_minimizer *r, size_t nr, int64_t len_r, int32_t init_len,
                                    const int32_t *limit, size_t n_limit, sdf_search_roll_rec *out) {
  if (nq == 0) return SDF_OK;
  const RollArgs A{q, nq, windows, first, intervals, r, nr, len_r, init_len, limit, n_limit};
  const char *why = nullptr;
  if (int rc = roll_arrays(A, out, &why)) return rc;
  ExtendMap S;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++) roll_one(A, i, intervals[t], out[t], S);
  return SDF_OK;
}

// ---- the extension ----

void sdf::extend_one(const ExtendArgs &A, size_t i, uint64_t t, sdf_search_hit &H, ExtendMap &S) {
  const RollArgs &RA = A.R;
  const sdf_search_window &W = RA.windows[i];
  const sdf_search_interval &T = RA.intervals[t];
  const sdf_search_roll_rec &Roll = A.rolls[t];
  const sdf_minimizer *q = RA.q, *r = RA.r;
  const int64_t nq = (int64_t)RA.nq, nr = (int64_t)RA.nr;
  H = sdf_search_hit{0, 0, 0, 0, 0, 0, 0, 0, 0, 0u};
  const int64_t lo = (int64_t)first_at_or_after(r, RA.nr, T.start);
  if (extend_skips(Roll, A.filter ? &A.filter[t] : nullptr, lo, nr)) {
    H.flags = SDF_EXTEND_SKIPPED;
    return;
  }
  bool wide = extend_replay_wide(Roll, W.n_members, lo), nolimit = false;
  // the entry state
  S.enter(q + i, W.n_members);
  const int64_t rws0 = Roll.winnow_start, rwe0 = Roll.winnow_end;
  roll_walk(RA, T, (size_t)lo, S, [&](int64_t, int64_t, size_t ws, size_t we) { return (int64_t)ws >= rws0 && (int64_t)we >= rwe0; });
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
    if (!S.has_B) S.to_first();
    else S.to_above();
    S.I += S.B_full();
  };
  const auto remove_from_query = [&](const sdf_minimizer &m) {
    if (!S.remove(search_host_key(m), 1, qsz != 0)) return;
    if (qsz > 0) --qsz;
    L = RA.limit[qsz];
    if (!S.has_B) return;
    S.I -= S.to_below();
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

// ---- the filter and its tasks ----

namespace {
// one side as the header states it: up, and its grams counted into hist
int32_t filter_side_host(const char *s, int32_t len, bool rc, std::vector<uint32_t> &hist) {
  int32_t up = 0;
  uint32_t g = 0;
  for (int32_t i = 0; i < len; i++) {
    unsigned char c = (unsigned char)(rc ? s[len - 1 - i] : s[i]) & 127;
    if (rc) c = (unsigned char)host_rev_dna((char)c);
    up += c >= 'A' && c <= 'Z';
    const unsigned char u = c & 0xDF;
    g = ((g << 2) | (u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u)) & (FILTER_GRAMS - 1);
    if (i >= 4) hist[g]++;
  }
  return up;
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

// (the tasks of the hits: the reference's second filter(), src/search.cc:356)
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

// ---- the found records: their bin entries, is_overlap ----

extern "C" int sdf_search_found_entries(const sdf_search_found *found, size_t nf, uint64_t *entries) {
  if (!entries || (nf && !found)) return SDF_ERR_INVALID;
  uint64_t n = 0;
  for (size_t f = 0; f < nf; f++)
    if (!found_empty(found[f])) n += (uint64_t)(found_bin((long long)found[f].q_end - 1) - found_bin(found[f].q_start) + 1);
  *entries = n;
  return SDF_OK;
}

extern "C" int sdf_search_overlap_host(const sdf_minimizer *q, size_t nq, const uint64_t *first, const sdf_search_roll_rec *rolls,
                                       const sdf_search_found *found, size_t nf, const uint32_t *visible_iv, int32_t init_len,
                                       int32_t min_read_size, uint32_t *out) {
  if (nq == 0) return SDF_OK;
  const char *why = nullptr;
  uint64_t entries = 0;
  if (int rc = overlap_arrays(q, nq, first, rolls, found, nf, visible_iv, init_len, min_read_size, out, &entries, &why)) return rc;
  for (size_t i = 0; i < nq; i++)
    for (uint64_t t = first[i]; t < first[i + 1]; t++)
      out[t] = found_any_overlap(found, visible_iv[t], q[i].loc, (long long)q[i].loc + init_len, rolls[t].ref_start, rolls[t].ref_end, min_read_size);
  return SDF_OK;
}

// ---- the acceptance step of a round ----

extern "C" int sdf_search_accept_host(const sdf_search_accept_round *R, sdf_search_found *found, size_t nf, size_t found_cap,
                                      sdf_search_pair_hit *out, size_t n_out, size_t out_cap, sdf_search_accept_status *status) {
  const char *why = nullptr;
  if (int rc = accept_scalars(R, found, nf, found_cap, out, n_out, out_cap, status, &why)) return rc;
  if (int rc = accept_arrays(R, &why)) return rc;
  struct Kept {
    uint64_t t;
    bool dropped;
  };
  std::vector<Kept> kept;  // of the windows in front of the frontier, in order
  std::vector<sdf_search_found> recs;
  int64_t attempted = 0, jaccard_failed = 0, interval_failed = 0;
  uint64_t n_found = 0, n_reported = 0;
  int32_t reach = 0;
  size_t frontier = R->na;
  bool incomplete = false;
  for (size_t j = 0; j < R->na; j++) {
    const size_t i = R->act[j];
    const long long pf_pos = R->q[i].loc, pf_end = pf_pos + R->init_len;
    const uint64_t t0 = R->first[i], t1 = R->first[i + 1];
    incomplete = t1 > R->n_max || (R->windows[i].flags & (SDF_SEARCH_WIDE | SDF_SEARCH_FOUND_WIDE));
    int64_t att = 0, jf = 0, ivf = 0;
    int32_t reach_w = 0;
    recs.clear();
    const size_t kept0 = kept.size();
    for (uint64_t t = t0; t < t1 && t1 <= R->n_max; t++) {
      const sdf_search_roll_rec &roll = R->rolls[t];
      const sdf_search_hit &H = R->hits[t];
      incomplete |= accept_unfinished(roll, H);
      att += 1;
      const int cls = accept_class(roll, R->overlap[t], R->filter[t], H, R->hit_filter[t]);
      if (cls == 0) jf += 1;
      if (cls == 1) ivf += 1;
      if (cls < 2) continue;
      if (found_any_overlap(recs.data(), recs.size(), pf_pos, pf_end, roll.ref_start, roll.ref_end, R->min_read_size)) {
        ivf += 1;
      } else if (cls == 3) {
        if (recs.size() < SDF_ACCEPT_MAX_KEPT) {
          recs.push_back(sdf_search_found{H.query_start, H.query_end, H.ref_start, H.ref_end});
          kept.push_back(Kept{t, false});
          reach_w = std::max(reach_w, H.query_end);
        } else {
          incomplete = true;
        }
      }
    }
    if (reach > pf_pos || incomplete) {
      kept.resize(kept0);
      frontier = j;
      break;
    }
    incomplete = false;
    const std::vector<uint8_t> dropped = parse_hits(recs.data(), recs.size());
    for (size_t h = 0; h < recs.size(); h++) kept[kept0 + h].dropped = dropped[h] != 0, n_reported += !dropped[h];
    n_found += recs.size();
    attempted += att, jaccard_failed += jf, interval_failed += ivf;
    reach = std::max(reach, reach_w);
  }
  sdf_search_accept_status S;
  S.need_found = nf + n_found, S.need_out = n_out + n_reported;
  const bool over = S.need_found > found_cap || S.need_out > out_cap;
  S.frontier = over ? 0u : (uint32_t)frontier;
  S.flags = over ? SDF_ACCEPT_OVERFLOW : incomplete ? SDF_ACCEPT_INCOMPLETE : 0u;
  S.nf = over ? nf : S.need_found, S.n_out = over ? n_out : S.need_out;
  S.attempted = over ? 0 : attempted, S.jaccard_failed = over ? 0 : jaccard_failed, S.interval_failed = over ? 0 : interval_failed;
  *status = S;
  if (over) return SDF_OK;
  // the append: window order, then interval order -- the order of `kept`
  size_t w = 0;
  for (size_t j = 0; j < frontier; j++) {
    const size_t i = R->act[j];
    for (; w < kept.size() && kept[w].t < R->first[i + 1]; w++) {
      const sdf_search_hit &H = R->hits[kept[w].t];
      found[nf++] = sdf_search_found{H.query_start, H.query_end, H.ref_start, H.ref_end};
      if (!kept[w].dropped)
        out[n_out++] = sdf_search_pair_hit{(int32_t)(R->window_base + (int32_t)i), H.query_start, H.query_end, H.ref_start, H.ref_end, H.jaccard};
    }
  }
  return SDF_OK;
}

// ---- initial_search, window by window ----

sdf::PairHostArgs sdf::pair_host_args(const char *pool, size_t pool_bytes, const sdf_minim_range &Q, const sdf_minim_range &R,
                                      const sdf_search_pair_params &P, const sdf_extend_params &E, const std::vector<sdf_minimizer> &q,
                                      const std::vector<sdf_minimizer> &r, const std::vector<sdf_minimizer> &r_sorted, uint32_t threshold) {
  return PairHostArgs{pool,          pool_bytes,         q.data(),   q.size(), r.data(), r_sorted.data(),
                      r.size(),      threshold,          Q.len,      R.len,    Q.off,    R.off,
                      (int)(Q.flags & SDF_MINIM_RC),     (int)(R.flags & SDF_MINIM_RC),  P.min_read_size,
                      P.same_genome != 0, P.uppercase_seeds != 0, P.limit, P.n_limit, P.filter, E};
}

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
  ExtendMap M;
  const size_t nf0 = found.size();
  const long long pf_pos = A.q[i].loc, pf_end = pf_pos + init_len;
  for (size_t t = 0; t < T.size(); t++) {
    W.attempted += 1;
    roll_one(RA, i, T[t], rolls[t], M);
    if (rolls[t].jaccard < 0) {
      W.jaccard_failed += 1;
      continue;
    }
    if (found_any_overlap(found.data(), found.size(), pf_pos, pf_end, rolls[t].ref_start, rolls[t].ref_end, A.min_read_size)) {
      W.interval_failed += 1;
      continue;
    }
    const sdf_filter_task task = filter_task_of(FA, pf_pos, win, T[t], rolls[t]);
    sdf_filter_rec rec;
    if (int rc = sdf_search_filter_host(A.pool, A.pool_bytes, &A.filter, &task, 1, &rec)) return rc;
    if (rec.flags & fail) continue;
    sdf_search_hit H;
    extend_one(EA, i, t, H, M);  // (a WIDE record is completed here, and is a hit)
    if (H.flags & (SDF_EXTEND_SKIPPED | SDF_EXTEND_NOLIMIT)) continue;
    const sdf_filter_task htask = hit_task_of(FA, H);
    if (int rc = sdf_search_filter_host(A.pool, A.pool_bytes, &A.filter, &htask, 1, &rec)) return rc;
    if (rec.flags & fail) continue;
    W.hits.push_back(sdf_search_pair_hit{(int32_t)i, H.query_start, H.query_end, H.ref_start, H.ref_end, H.jaccard});
    found.push_back(sdf_search_found{H.query_start, H.query_end, H.ref_start, H.ref_end});
  }
  // (the window's hits are the records it appended, in order)
  const std::vector<uint8_t> dropped = parse_hits(found.data() + nf0, W.hits.size());
  for (size_t h = 0; h < W.hits.size(); h++)
    if (!dropped[h]) W.reported.push_back(W.hits[h]);
  return SDF_OK;
}

namespace {
// the sequence of a range: its characters & 127, reverse-complemented by rev_dna under SDF_MINIM_RC
std::string host_sequence(const char *pool, const sdf_minim_range &r) {
  std::string s((size_t)r.len, 'N');
  for (int32_t x = 0; x < r.len; x++) {
    const char c = (char)(pool[r.off + x] & 127);
    if (r.flags & SDF_MINIM_RC) s[(size_t)(r.len - 1 - x)] = host_rev_dna(c);
    else s[(size_t)x] = c;
  }
  return s;
}
// get_minimizers (src/hash.cc:53-100) as tests/minim_model.py holds it, the deque loop as written
std::vector<sdf_minimizer> host_minimizers(const std::string &s, int k, int w, bool separate_lowercase) {
  std::vector<sdf_minimizer> out;
  struct Item {
    uint64_t key;
    int64_t loc;
  };
  std::deque<Item> window;
  const uint32_t mask = (uint32_t)((1ull << (2 * k)) - 1);
  uint32_t h = 0;
  int64_t last_n = -(int64_t)k - w, last_u = last_n;
  for (int64_t i = 0; i < (int64_t)s.size(); i++) {
    const char c = s[(size_t)i];
    if (c == 'N' || c == 'n') last_n = i;
    else if (c >= 'A' && c <= 'Z') last_u = i;
    const uint32_t code = c == 'C' || c == 'c' ? 1u : c == 'G' || c == 'g' ? 2u : c == 'T' || c == 't' ? 3u : 0u;
    h = ((h << 2) | code) & mask;
    if (i < k - 1) continue;
    const int64_t at = i - k + 1;
    uint32_t status = last_n >= at ? 2u : last_u >= at ? 0u : 1u;
    if (!separate_lowercase && status == 1u) status = 0u;
    const uint64_t key = (uint64_t)status << 32 | h;
    while (!window.empty() && !(window.back().key < key)) window.pop_back();
    while (!window.empty() && window.back().loc < at - w) window.pop_front();
    window.push_back(Item{key, at});
    if (at < w) continue;
    const Item &f = window.front();
    if (out.empty() || !((int64_t)out.back().loc == f.loc && search_host_key(out.back()) == f.key))
      out.push_back(sdf_minimizer{(uint32_t)f.key, (int32_t)f.loc, (int32_t)(f.key >> 32), 0});
  }
  return out;
}
// Index::Index (src/hash.cc:113-141): the records in ascending (status, hash, loc), and the threshold
uint32_t host_index(const std::vector<sdf_minimizer> &m, std::vector<sdf_minimizer> &sorted) {
  sorted = m;
  std::stable_sort(sorted.begin(), sorted.end(), [](const sdf_minimizer &a, const sdf_minimizer &b) { return search_host_key(a) < search_host_key(b); });
  std::map<uint64_t, uint64_t> hist;  // group size -> groups
  for (size_t a = 0; a < sorted.size();) {
    size_t b = a;
    while (b < sorted.size() && search_host_key(sorted[b]) == search_host_key(sorted[a])) ++b;
    hist[b - a] += 1;
    a = b;
  }
  const int ignore = (int)(((double)m.size() * 0.001) / 100.0);
  uint64_t total = 0;
  uint32_t threshold = 0x80000000u;
  for (auto it = hist.rbegin(); it != hist.rend(); ++it) {
    total += it->second;
    if (total > (uint64_t)ignore) break;
    threshold = (uint32_t)it->first;
  }
  return threshold;
}
}  // namespace

extern "C" int sdf_search_pair_host(const char *pool, size_t pool_bytes, const sdf_minim_range *q_range, const sdf_minim_range *r_range,
                                    const sdf_search_pair_params *params, sdf_search_pair_hit *out, size_t cap, size_t *used,
                                    sdf_search_pair_stats *stats) {
  if (!used || !stats || (cap && !out) || (pool_bytes && !pool)) return SDF_ERR_INVALID;
  if (int rc = pair_checks(pool_bytes, q_range, r_range, params)) return rc;
  const sdf_search_pair_params &P = *params;
  const std::string qs = host_sequence(pool, *q_range);
  const std::vector<sdf_minimizer> q = host_minimizers(qs, P.k, P.w, P.separate_lowercase != 0);
  std::vector<sdf_minimizer> r_own, r_sorted;
  if (!P.same_genome) r_own = host_minimizers(host_sequence(pool, *r_range), P.k, P.w, P.separate_lowercase != 0);
  const std::vector<sdf_minimizer> &r = P.same_genome ? q : r_own;
  const uint32_t threshold = host_index(r, r_sorted);
  const PairHostArgs A = pair_host_args(pool, pool_bytes, *q_range, *r_range, P, pair_extend_params(P), q, r, r_sorted, threshold);
  std::vector<sdf_search_found> found;
  std::vector<sdf_search_pair_hit> all;
  PairHostWindow W;
  sdf_search_pair_stats S{0, 0, 0, 0, 0, 0, 0};
  int64_t next = 0;
  for (size_t i = 0; i < q.size(); i++) {
    if ((int64_t)q[i].loc < next) continue;
    if (P.uppercase_seeds && q[i].status != 0) continue;
    if (int rc = pair_host_window(A, i, found, W)) return rc;
    S.attempted += W.attempted, S.jaccard_failed += W.jaccard_failed, S.interval_failed += W.interval_failed;
    S.windows_run += 1, S.windows_scheduled += 1, S.windows_host += 1;
    int64_t min_len = q_range->len;
    for (const sdf_search_pair_hit &h : W.reported) min_len = std::min<int64_t>(min_len, (int64_t)h.query_end - h.query_start);
    all.insert(all.end(), W.reported.begin(), W.reported.end());
    next = min_len >= P.min_read_size ? pair_next_loc(q[i].loc, P.min_read_size, P.filter.max_error) : (int64_t)q[i].loc;
  }
  *stats = S;
  *used = all.size();
  if (all.size() > cap) return SDF_ERR_CIGAR_OVERFLOW;
  if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(sdf_search_pair_hit));
  return SDF_OK;
}
