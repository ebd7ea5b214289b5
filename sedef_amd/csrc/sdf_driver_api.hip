// The C ABI: the search driver (include/sedef_hip.h states the rules) -- the device and uploading forms of a round's
// acceptance step (search_accept.hip) with their launches, and sdf_search_pair, the stages and the acceptance step in rounds
// on the resident pool; the resident search index (sdf_search_index_*) and sdf_search_pair_indexed, the same rounds on two
// handles.  sdf_search_accept_host, sdf_search_pair_host, the window that sdf_search_pair hands to the host
// (pair_host_window) and the checks: search_host.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "sdf_entry.h"
#include "search_host.h"

using namespace sdf;

namespace {
// the three launches on `st` (one when the round is empty)
int accept_launch(sdf_ctx *ctx, const sdf_search_accept_round *R, sdf_search_found *d_found, size_t nf, size_t found_cap,
                  sdf_search_pair_hit *d_out, size_t n_out, size_t out_cap, sdf_search_accept_status *d_status, hipStream_t st) {
  const size_t na = R->na;
  SDF_HIP(ctx->ac_win.reserve((na + 1) * sizeof(AcceptWin)));
  SDF_HIP(ctx->ac_off.reserve((na + 1) * sizeof(AcceptOff)));
  SDF_HIP(ctx->ac_kept.reserve((R->n_max + 1) * 4));
  SDF_HIP(ctx->ac_go.reserve(4));
  const AcceptRound A{R->q,    R->act,        R->windows,         R->first,    R->rolls,     R->overlap,          R->filter,
                      R->hits, R->hit_filter, (long long)R->n_max, (int)R->nq, (int)na, (int)R->init_len, (int)R->min_read_size, (int)R->window_base};
  AcceptWin *d_win = (AcceptWin *)ctx->ac_win.p;
  AcceptOff *d_off = (AcceptOff *)ctx->ac_off.p;
  uint32_t *d_kept = (uint32_t *)ctx->ac_kept.p, *d_go = (uint32_t *)ctx->ac_go.p;
  if (na) hipLaunchKernelGGL(search_accept_window_kernel, dim3((unsigned)na), dim3(64), 0, st, A, d_win, d_kept);
  hipLaunchKernelGGL(search_accept_frontier_kernel, dim3(1), dim3(1024), 0, st, (const AcceptWin *)d_win, (int)na, (unsigned long long)nf,
                     (unsigned long long)found_cap, (unsigned long long)n_out, (unsigned long long)out_cap, d_off, d_status, d_go);
  if (na)
    hipLaunchKernelGGL(search_accept_append_kernel, dim3((unsigned)na), dim3(64), 0, st, A, (const AcceptWin *)d_win, (const uint32_t *)d_kept,
                       (const AcceptOff *)d_off, (const uint32_t *)d_go, d_found, (unsigned long long)nf, (unsigned long long)found_cap, d_out,
                       (unsigned long long)n_out, (unsigned long long)out_cap);
  SDF_HIP(hipGetLastError());
  ctx->launches += na ? 3 : 1;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_accept_device(sdf_ctx *ctx, const sdf_search_accept_round *R, sdf_search_found *d_found, size_t nf, size_t found_cap,
                                        sdf_search_pair_hit *d_out, size_t n_out, size_t out_cap, sdf_search_accept_status *d_status,
                                        void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = nullptr;
  if (int rc = accept_scalars(R, d_found, nf, found_cap, d_out, n_out, out_cap, d_status, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (int rc = accept_launch(ctx, R, d_found, nf, found_cap, d_out, n_out, out_cap, d_status, st)) return rc;
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_search_accept(sdf_ctx *ctx, const sdf_search_accept_round *R, sdf_search_found *found, size_t nf, size_t found_cap,
                                 sdf_search_pair_hit *out, size_t n_out, size_t out_cap, sdf_search_accept_status *status) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = nullptr;
  if (int rc = accept_scalars(R, found, nf, found_cap, out, n_out, out_cap, status, &why)) return refuse(ctx, rc, why);
  if (int rc = accept_arrays(R, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the round's arrays in one piece; the per-interval ones hold what the windows name and no more than n_max
  const size_t n = R->na ? (size_t)std::min<uint64_t>(R->first[R->nq], R->n_max) : 0, nq = R->na ? R->nq : 0;
  struct Piece {
    const void *src;
    size_t bytes, at;
  } P[] = {{R->q, nq * sizeof(sdf_minimizer), 0},        {R->act, R->na * 4, 0},
           {R->windows, nq * sizeof(sdf_search_window), 0}, {R->first, R->na ? (nq + 1) * 8 : 0, 0},
           {R->rolls, n * sizeof(sdf_search_roll_rec), 0},  {R->overlap, n * 4, 0},
           {R->filter, n * sizeof(sdf_filter_rec), 0},      {R->hits, n * sizeof(sdf_search_hit), 0},
           {R->hit_filter, n * sizeof(sdf_filter_rec), 0}};
  size_t total = 0;
  for (Piece &p : P) p.at = total, total += (p.bytes + 255) / 256 * 256;
  SDF_HIP(ctx->ac_in.reserve(total + 256));
  SDF_HIP(ctx->ac_found.reserve((found_cap + 1) * sizeof(sdf_search_found)));
  SDF_HIP(ctx->ac_out.reserve((out_cap + 1) * sizeof(sdf_search_pair_hit)));
  SDF_HIP(ctx->ac_status.reserve(sizeof(sdf_search_accept_status)));
  uint8_t *base = (uint8_t *)ctx->ac_in.p;
  for (const Piece &p : P)
    if (p.bytes) SDF_HIP(hipMemcpyAsync(base + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
  if (nf) SDF_HIP(hipMemcpyAsync(ctx->ac_found.p, found, nf * sizeof(sdf_search_found), hipMemcpyHostToDevice, st));
  sdf_search_accept_round D = *R;
  D.q = (const sdf_minimizer *)(base + P[0].at), D.act = (const uint32_t *)(base + P[1].at);
  D.windows = (const sdf_search_window *)(base + P[2].at), D.first = (const uint64_t *)(base + P[3].at);
  D.rolls = (const sdf_search_roll_rec *)(base + P[4].at), D.overlap = (const uint32_t *)(base + P[5].at);
  D.filter = (const sdf_filter_rec *)(base + P[6].at), D.hits = (const sdf_search_hit *)(base + P[7].at);
  D.hit_filter = (const sdf_filter_rec *)(base + P[8].at);
  D.n_max = n;  // (a window whose records lie beyond R->n_max has them beyond n too)
  sdf_search_found *d_found = (sdf_search_found *)ctx->ac_found.p;
  sdf_search_pair_hit *d_out = (sdf_search_pair_hit *)ctx->ac_out.p;
  if (int rc = accept_launch(ctx, &D, d_found, nf, found_cap, d_out, n_out, out_cap, (sdf_search_accept_status *)ctx->ac_status.p, st)) return rc;
  SDF_HIP(hipMemcpyAsync(status, ctx->ac_status.p, sizeof *status, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  if (status->nf > nf)
    SDF_HIP(hipMemcpyAsync(found + nf, d_found + nf, (size_t)(status->nf - nf) * sizeof(sdf_search_found), hipMemcpyDeviceToHost, st));
  if (status->n_out > n_out)
    SDF_HIP(hipMemcpyAsync(out + n_out, d_out + n_out, (size_t)(status->n_out - n_out) * sizeof(sdf_search_pair_hit), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// ---- sdf_search_pair: the stages and the acceptance step in rounds, on the resident pool ----

namespace {
constexpr size_t kPairRoundWindows = SDF_PAIR_ROUND_WINDOWS;  // round_windows == 0; not measured (profiles/search_driver.py has the sweep)
// long growths a round finishes on the device; the host takes the rest
constexpr size_t kPairLongMax = SDF_PAIR_LONG_MAX, kPairLongBatch = SDF_PAIR_LONG_BATCH;

struct PairDriver {
  sdf_ctx *ctx;
  hipStream_t st;
  const sdf_search_pair_params &P;
  const sdf_extend_params E;  // P.extend as the stages take it
  sdf_minim_range Q, R;
  // the query's minimizers and the reference's (the query's own under same_genome) in ascending loc, the reference's index:
  // the host's copies and the device's -- the call's own (sdf_search_pair) or two handles' (sdf_search_pair_indexed)
  const std::vector<sdf_minimizer> *q = nullptr, *r_loc = nullptr, *r_sorted = nullptr;
  const sdf_minimizer *d_q = nullptr, *d_r = nullptr, *d_rs = nullptr;
  uint32_t threshold = 0x80000000u;
  std::vector<sdf_search_found> found;  // the host's mirror of the device list
  std::vector<sdf_search_pair_hit> out;
  std::string chars;  // both ranges as they lie in the pool, fetched when the host first completes a window
  PairHostWindow W;
  sdf_search_pair_stats S{0, 0, 0, 0, 0, 0, 0};
  size_t cap_iv = SDF_PAIR_INTERVALS_START, ent_cap = SDF_PAIR_ENTRIES_START, found_cap = 0;
  size_t n_wide = 0;  // sdf_search_pair_wide: the n_wide_max of a round's seeding (0: the plain device form)
  const std::vector<sdf_minimizer> &r() const { return *r_loc; }
};

int pair_minimizers(sdf_ctx *ctx, const sdf_minim_range &range, int k, int w, int separate_lowercase, bool index, std::vector<sdf_minimizer> &out,
                    uint32_t *threshold, uint32_t *n_groups = nullptr) {
  uint64_t first[2] = {0, 0};
  uint32_t groups = 0, thr = 0;
  size_t used = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int rc = index ? sdf_pool_minimizer_index(ctx, &range, 1, k, w, separate_lowercase, first, out.data(), out.size(), &used, &groups, &thr)
                         : sdf_pool_minimizers(ctx, &range, 1, k, w, separate_lowercase, first, out.data(), out.size(), &used);
    if (rc == SDF_OK) break;
    if (rc != SDF_ERR_CIGAR_OVERFLOW || pass) return rc;
    out.resize(used);
  }
  out.resize(used);
  if (threshold) *threshold = thr;
  if (n_groups) *n_groups = groups;
  return SDF_OK;
}

// the device list behind the host's mirror: room for `want` records, records [from, found.size()) uploaded
int pair_sync_found(PairDriver &D, size_t want, size_t from) {
  sdf_ctx *ctx = D.ctx;
  if (want > D.found_cap) {
    D.found_cap = 2 * want + 1024;
    SDF_HIP(ctx->dr_found.reserve(D.found_cap * sizeof(sdf_search_found)));
    from = 0;  // (a buffer that grew is a new one)
  }
  if (D.found.size() > from)
    SDF_HIP(hipMemcpyAsync((sdf_search_found *)ctx->dr_found.p + from, D.found.data() + from, (D.found.size() - from) * sizeof(sdf_search_found),
                           hipMemcpyHostToDevice, D.st));
  return SDF_OK;
}

// window i by the per-window step of sdf_search_pair_host, its records to both lists
int pair_host_one(PairDriver &D, size_t i) {
  sdf_ctx *ctx = D.ctx;
  if (D.chars.empty()) {
    D.chars.resize((size_t)D.Q.len + (D.P.same_genome ? 0 : (size_t)D.R.len));
    const sdf_pool_fetch F[2] = {{D.Q.off, D.Q.len, 0, 0}, {D.R.off, D.R.len, 0, D.Q.len}};
    if (int rc = sdf_pool_fetch_ranges(ctx, F, D.P.same_genome ? 1 : 2, &D.chars[0], D.chars.size())) return rc;
  }
  // (the ranges as they lie in chars)
  const sdf_minim_range Q{0, D.Q.len, D.Q.flags}, R{D.P.same_genome ? 0 : (int64_t)D.Q.len, D.R.len, D.R.flags};
  const PairHostArgs A = pair_host_args(D.chars.data(), D.chars.size(), Q, R, D.P, D.E, *D.q, D.r(), *D.r_sorted, D.threshold);
  const size_t nf0 = D.found.size();
  if (int rc = pair_host_window(A, i, D.found, D.W)) return refuse(ctx, rc, "sdf_search_pair: the host step of a window failed");
  D.out.insert(D.out.end(), D.W.reported.begin(), D.W.reported.end());
  D.S.attempted += D.W.attempted, D.S.jaccard_failed += D.W.jaccard_failed, D.S.interval_failed += D.W.interval_failed;
  D.S.windows_host += 1, D.S.windows_run += 1;
  return pair_sync_found(D, D.found.size(), nf0);
}

// One round over the scheduled windows act[0, na) (ascending indices into q): the chain on the context's stream, one wait.
// *status: the acceptance step's; *grew: a capacity was short and has been raised -- the status is then not to be used.
int pair_round(PairDriver &D, const uint32_t *act, size_t na, sdf_search_accept_status *status, bool *grew) {
  sdf_ctx *ctx = D.ctx;
  hipStream_t st = D.st;
  const sdf_search_pair_params &P = D.P;
  const size_t nq = D.q->size(), nr = D.r().size(), nf = D.found.size(), n = D.cap_iv;
  const std::vector<sdf_minimizer> &q = *D.q;
  const int32_t init_len = P.min_read_size;
  const int64_t len_q = D.Q.len, len_r = D.R.len;
  const int q_rc = (int)(D.Q.flags & SDF_MINIM_RC), r_rc = (int)(D.R.flags & SDF_MINIM_RC);
  // the slice of q the round's windows and their members lie in
  const size_t i0 = act[0];
  size_t e = act[na - 1];
  while (e < nq && (int64_t)q[e].loc - q[act[na - 1]].loc <= init_len) ++e;
  const size_t ns = e - i0;
  if (int rc = pair_sync_found(D, nf + n, nf)) return rc;
  SDF_HIP(ctx->dr_vis.reserve((std::max(nq, n) + 1) * 4));
  SDF_HIP(ctx->dr_iv.reserve((n + 1) * sizeof(sdf_search_interval)));
  SDF_HIP(ctx->dr_rolls.reserve((n + 1) * sizeof(sdf_search_roll_rec)));
  SDF_HIP(ctx->dr_tasks.reserve((n + 1) * sizeof(sdf_filter_task)));
  SDF_HIP(ctx->dr_verd.reserve((n + 1) * 4));
  SDF_HIP(ctx->dr_frec.reserve((n + 1) * sizeof(sdf_filter_rec)));
  SDF_HIP(ctx->dr_hits.reserve((n + 1) * sizeof(sdf_search_hit)));
  SDF_HIP(ctx->dr_htasks.reserve((n + 1) * sizeof(sdf_filter_task)));
  SDF_HIP(ctx->dr_hrec.reserve((n + 1) * sizeof(sdf_filter_rec)));
  SDF_HIP(ctx->dr_out.reserve((n + 1) * sizeof(sdf_search_pair_hit)));
  SDF_HIP(ctx->dr_status.reserve(sizeof(sdf_search_accept_status) + 16));
  if (int rc = upload_all(ctx, st, {{ctx->dr_act, act, na * 4}})) return rc;
  const sdf_minimizer *d_q = D.d_q, *d_r = D.d_r, *d_rs = D.d_rs;
  const int32_t *d_limit = (const int32_t *)ctx->dr_limit.p;
  uint64_t *d_first = (uint64_t *)ctx->dr_first.p;
  sdf_search_window *d_win = (sdf_search_window *)ctx->dr_win.p;
  uint32_t *d_vis = (uint32_t *)ctx->dr_vis.p, *d_verd = (uint32_t *)ctx->dr_verd.p;
  sdf_search_interval *d_iv = (sdf_search_interval *)ctx->dr_iv.p;
  sdf_search_roll_rec *d_rolls = (sdf_search_roll_rec *)ctx->dr_rolls.p;
  sdf_filter_task *d_tasks = (sdf_filter_task *)ctx->dr_tasks.p, *d_htasks = (sdf_filter_task *)ctx->dr_htasks.p;
  sdf_filter_rec *d_frec = (sdf_filter_rec *)ctx->dr_frec.p, *d_hrec = (sdf_filter_rec *)ctx->dr_hrec.p;
  sdf_search_hit *d_hits = (sdf_search_hit *)ctx->dr_hits.p;
  sdf_search_found *d_found = (sdf_search_found *)ctx->dr_found.p;
  sdf_search_accept_status *d_status = (sdf_search_accept_status *)ctx->dr_status.p;
  uint64_t *d_need = (uint64_t *)(d_status + 1);
  const sdf_extend_params &E = D.E;
  void *s = (void *)st;
  // every window and interval of the round sees the whole list as it stands
  SDF_HIP(hipMemsetD32Async((hipDeviceptr_t)d_vis, (int)nf, std::max(nq, n), st));
  if (i0) SDF_HIP(hipMemsetAsync(d_first, 0, i0 * 8, st));
  if (int rc = D.n_wide ? sdf_search_windows_wide_device(ctx, d_q + i0, ns, len_q, d_rs, nr, D.threshold, init_len, P.same_genome, P.uppercase_seeds,
                                                         d_limit, P.n_limit, d_found, nf, D.ent_cap, d_need, d_vis, d_first + i0, d_win + i0, d_iv, n,
                                                         nullptr, D.n_wide, nullptr, s)
                        : sdf_search_windows_found_device(ctx, d_q + i0, ns, len_q, d_rs, nr, D.threshold, init_len, P.same_genome, P.uppercase_seeds,
                                                          d_limit, P.n_limit, d_found, nf, D.ent_cap, d_need, d_vis, d_first + i0, d_win + i0, d_iv, n,
                                                          nullptr, s))
    return rc;
  if (e < nq) {
    hipLaunchKernelGGL(search_accept_tail_kernel, dim3((unsigned)((nq - e + 255) / 256)), dim3(256), 0, st, d_first, (int)e, (int)nq);
    SDF_HIP(hipGetLastError());
    ctx->launches += 1;
  }
  if (int rc = sdf_search_roll_device(ctx, d_q, nq, d_win, d_first, d_iv, n, d_r, nr, len_r, init_len, d_limit, P.n_limit, d_rolls, s)) return rc;
  if (int rc = sdf_search_filter_tasks_device(ctx, d_q, nq, d_win, d_first, d_iv, d_rolls, n, len_q, len_r, init_len, D.Q.off, q_rc, D.R.off, r_rc, 1,
                                              d_tasks, s))
    return rc;
  if (int rc = sdf_search_overlap_device(ctx, d_q, nq, d_first, d_rolls, n, d_found, nf, D.ent_cap, nullptr, d_vis, init_len, P.min_read_size, d_verd,
                                         d_tasks, s))
    return rc;
  if (int rc = sdf_search_filter_device(ctx, &P.filter, d_tasks, n, q_rc | r_rc, d_frec, s)) return rc;
  if (int rc = sdf_search_extend_device(ctx, d_q, nq, d_win, d_first, d_iv, d_rolls, d_frec, n, d_r, nr, len_q, len_r, init_len, d_limit, P.n_limit, &E,
                                        d_hits, s))
    return rc;
  {  // long growths; without room for its workspace the host completes them
    const int rc = sdf_search_extend_long_device(ctx, d_q, nq, d_win, d_first, d_iv, d_rolls, d_frec, n, d_r, nr, len_q, len_r, init_len, d_limit,
                                                 P.n_limit, &E, SDF_EXTEND_LONG_MAX_GROW, kPairLongMax, kPairLongBatch, d_hits, nullptr, s);
    if (rc != SDF_OK && rc != SDF_ERR_NOMEM) return rc;
  }
  if (int rc = sdf_search_hit_tasks_device(ctx, d_hits, n, d_first + nq, len_q, len_r, D.Q.off, q_rc, D.R.off, r_rc, d_htasks, s)) return rc;
  if (int rc = sdf_search_filter_device(ctx, &P.filter, d_htasks, n, q_rc | r_rc, d_hrec, s)) return rc;
  const sdf_search_accept_round A{d_q,   nq,     (const uint32_t *)ctx->dr_act.p, na,     d_win,  d_first,          n,          d_rolls,
                                  d_verd, d_frec, d_hits,                          d_hrec, init_len, P.min_read_size, 0, 0};
  if (int rc = sdf_search_accept_device(ctx, &A, d_found, nf, D.found_cap, (sdf_search_pair_hit *)ctx->dr_out.p, 0, n, d_status, s)) return rc;
  SDF_HIP(hipMemcpyAsync(d_need + 1, d_first + nq, 8, hipMemcpyDeviceToDevice, st));
  struct {
    sdf_search_accept_status status;
    uint64_t entries, intervals;
  } back;
  SDF_HIP(hipMemcpyAsync(&back, d_status, sizeof back, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));  // the round's one wait
  D.S.rounds += 1, D.S.windows_run += (int64_t)na;
  *grew = false;
  if (back.entries > D.ent_cap) D.ent_cap = 2 * (size_t)back.entries, *grew = true;  // the index was incomplete: nothing of the round holds
  if (back.intervals > n && (*grew || back.status.frontier == 0)) D.cap_iv = 2 * (size_t)back.intervals, *grew = true;
  else if (back.intervals > n) D.cap_iv = 2 * (size_t)back.intervals;  // (the windows whose records were there are taken; the next round has room)
  if (back.status.flags & SDF_ACCEPT_OVERFLOW) return refuse(ctx, SDF_ERR_HIP, "sdf_search_pair: internal error, a round overflowed lists sized for it");
  if (back.intervals > n) back.status.flags &= ~(uint32_t)SDF_ACCEPT_INCOMPLETE;  // (incomplete for want of room, not for the host)
  *status = back.status;
  if (*grew) return SDF_OK;
  // the round's new records, to the host's mirrors
  const size_t add_f = (size_t)(back.status.nf - nf), add_o = (size_t)back.status.n_out;
  D.found.resize(nf + add_f);
  const size_t o0 = D.out.size();
  D.out.resize(o0 + add_o);
  if (add_f) SDF_HIP(hipMemcpyAsync(D.found.data() + nf, d_found + nf, add_f * sizeof(sdf_search_found), hipMemcpyDeviceToHost, st));
  if (add_o) SDF_HIP(hipMemcpyAsync(D.out.data() + o0, ctx->dr_out.p, add_o * sizeof(sdf_search_pair_hit), hipMemcpyDeviceToHost, st));
  if (add_f || add_o) SDF_HIP(hipStreamSynchronize(st));
  D.S.attempted += back.status.attempted, D.S.jaccard_failed += back.status.jaccard_failed, D.S.interval_failed += back.status.interval_failed;
  return SDF_OK;
}

// fact 1: the windows that run, from loc and status alone
void pair_schedule(PairDriver &D, std::vector<uint32_t> &sched) {
  const sdf_search_pair_params &P = D.P;
  const std::vector<sdf_minimizer> &q = *D.q;
  int64_t next = 0;
  for (size_t i = 0; i < q.size(); i++) {
    if ((int64_t)q[i].loc < next || (P.uppercase_seeds && q[i].status != 0)) continue;
    sched.push_back((uint32_t)i);
    next = pair_next_loc(q[i].loc, P.min_read_size, P.filter.max_error);
  }
  D.S.windows_scheduled = (int64_t)sched.size();
}

// The rounds over a schedule that is not empty; D.d_q, D.d_r and D.d_rs name the device copies.  What a call writes per
// window -- first[], the window records -- lies in the context's own buffers, never with the minimizers.
int pair_rounds(PairDriver &D, const std::vector<uint32_t> &sched) {
  sdf_ctx *ctx = D.ctx;
  hipStream_t st = D.st;
  const sdf_search_pair_params &P = D.P;
  const size_t nq = D.q->size();
  // (an array without a record still gets a buffer: the device forms -- sdf_search_roll_device's d_r and d_limit first -- refuse a null
  // pointer before they look at a count)
  SDF_HIP(ctx->dr_limit.reserve(16));
  if (int rc = upload_all(ctx, st, {{ctx->dr_limit, P.limit, P.n_limit * 4}})) return rc;
  SDF_HIP(ctx->dr_first.reserve((nq + 1) * 8));
  SDF_HIP(ctx->dr_win.reserve((nq + 1) * sizeof(sdf_search_window)));
  SDF_HIP(hipMemsetAsync(ctx->dr_win.p, 0, nq * sizeof(sdf_search_window), st));
  const size_t round = P.round_windows ? P.round_windows : kPairRoundWindows, every = P.debug_host_every;
  size_t s0 = 0;
  while (s0 < sched.size()) {
    if (every && s0 % every == every - 1) {  // debug: this window on the host
      if (int rc = pair_host_one(D, sched[s0])) return rc;
      ++s0;
      continue;
    }
    size_t na = std::min(round, sched.size() - s0);
    if (every) na = std::min(na, every - 1 - s0 % every);  // (the round ends in front of the next one the host takes)
    sdf_search_accept_status status;
    bool grew = false;
    if (int rc = pair_round(D, sched.data() + s0, na, &status, &grew)) return rc;
    if (grew) continue;  // the same round again, with room
    s0 += status.frontier;
    if (status.flags & SDF_ACCEPT_INCOMPLETE) {
      if (int rc = pair_host_one(D, sched[s0])) return rc;
      ++s0;
    } else if (status.frontier == 0) {
      return refuse(ctx, SDF_ERR_HIP, "sdf_search_pair: internal error, a round accepted nothing and handed nothing to the host");
    }
  }
  return SDF_OK;
}

int pair_finish(sdf_ctx *ctx, const std::vector<sdf_search_pair_hit> &hits, sdf_search_pair_hit *out, size_t cap, size_t *used) {
  *used = hits.size();
  if (hits.size() > cap) return refuse(ctx, SDF_ERR_CIGAR_OVERFLOW, "the pair has " + std::to_string(hits.size()) + " hits, more than cap");
  if (!hits.empty()) memcpy(out, hits.data(), hits.size() * sizeof(sdf_search_pair_hit));
  return SDF_OK;
}

// a handle this context holds (looked up by address: a freed handle or another context's is not read)
bool index_live(const sdf_ctx *ctx, const sdf_search_index *h) {
  return h && std::find(ctx->indexes.begin(), ctx->indexes.end(), h) != ctx->indexes.end();
}
}  // namespace

// ---- two handles as a pair: the checks and the rounds, for the single-pair calls below and for the lanes (sdf_lanes_api.hip).
// `owner` holds the handles; the rounds run on `ctx` -- the owner itself, or a lane that views the owner's pool.
namespace sdf {
int pair_handles_valid(const sdf_ctx *owner, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                       const char **why) {
  if (!index_live(owner, q) || !index_live(owner, r))
    return *why = "sdf_search_pair_indexed: a handle that is null, freed or another context's", SDF_ERR_INVALID;
  if (q->pool_epoch != owner->pool_epoch || r->pool_epoch != owner->pool_epoch)
    return *why = "sdf_search_pair_indexed: a handle built on a pool that has been replaced since", SDF_ERR_INVALID;
  for (const sdf_search_index *h : {q, r})
    if (h->k != params->k || h->w != params->w || h->separate_lowercase != (params->separate_lowercase != 0))
      return *why = "sdf_search_pair_indexed: k, w or separate_lowercase differ from a handle's", SDF_ERR_INVALID;
  if (params->same_genome && q != r) return *why = "sdf_search_pair_indexed: same_genome takes one handle as both sides", SDF_ERR_INVALID;
  return SDF_OK;
}

int pair_handles_ranges(size_t pool_bytes, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                        size_t n_wide_max, const char **why) {
  if (int rc = pair_checks(pool_bytes, &q->range, &r->range, params))
    return *why = "sdf_search_pair_indexed: a range or a parameter is refused", rc;
  if (n_wide_max > SEARCH_WIDE_MAX_LIST) return *why = "sdf_search_pair_indexed_wide: n_wide_max > 2^20", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

int pair_handles_run(sdf_ctx *ctx, const sdf_ctx *owner, const sdf_search_index *q, const sdf_search_index *r,
                     const sdf_search_pair_params *params, size_t n_wide_max, std::vector<sdf_search_pair_hit> &hits,
                     sdf_search_pair_stats *stats) {
  ctx->err.clear();
  const char *why = nullptr;
  if (int rc = pair_handles_valid(owner, q, r, params, &why)) return refuse(ctx, rc, why);
  if (int rc = pair_handles_ranges(sdf_pool_bytes(ctx), q, r, params, n_wide_max, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  PairDriver D{ctx, ctx->stream, *params, pair_extend_params(*params), q->range, r->range};
  D.n_wide = n_wide_max;
  D.q = &q->loc, D.r_loc = &r->loc, D.r_sorted = &r->sorted, D.threshold = r->threshold;
  D.d_q = (const sdf_minimizer *)q->d_loc.p, D.d_r = (const sdf_minimizer *)r->d_loc.p, D.d_rs = (const sdf_minimizer *)r->d_sorted.p;
  std::vector<uint32_t> sched;
  pair_schedule(D, sched);
  if (!sched.empty())
    if (int rc = pair_rounds(D, sched)) return rc;
  *stats = D.S;
  hits.swap(D.out);
  return SDF_OK;
}
}  // namespace sdf

// sdf_search_pair (n_wide_max == 0) and sdf_search_pair_wide
static int pair_ranges(sdf_ctx *ctx, const sdf_minim_range *q_range, const sdf_minim_range *r_range, const sdf_search_pair_params *params,
                       sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats, size_t n_wide_max) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!used || !stats || (cap && !out)) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_pair: invalid arguments");
  if (int rc = pair_checks(sdf_pool_bytes(ctx), q_range, r_range, params)) return refuse(ctx, rc, "sdf_search_pair: a range or a parameter is refused");
  if (n_wide_max > SEARCH_WIDE_MAX_LIST) return refuse(ctx, SDF_ERR_UNSUPPORTED, "sdf_search_pair_wide: n_wide_max > 2^20");
  SDF_HIP(hipSetDevice(ctx->device));
  PairDriver D{ctx, ctx->stream, *params, pair_extend_params(*params), *q_range, *r_range};
  D.n_wide = n_wide_max;
  const sdf_search_pair_params &P = *params;
  // set-up: minimizers of both ranges, the reference's index; they stay in HBM for every round
  std::vector<sdf_minimizer> q, r_own, r_sorted;
  if (int rc = pair_minimizers(ctx, D.Q, P.k, P.w, P.separate_lowercase, false, q, nullptr)) return rc;
  if (!P.same_genome)
    if (int rc = pair_minimizers(ctx, D.R, P.k, P.w, P.separate_lowercase, false, r_own, nullptr)) return rc;
  if (int rc = pair_minimizers(ctx, D.R, P.k, P.w, P.separate_lowercase, true, r_sorted, &D.threshold)) return rc;
  D.q = &q, D.r_loc = P.same_genome ? &q : &r_own, D.r_sorted = &r_sorted;
  std::vector<uint32_t> sched;
  pair_schedule(D, sched);
  if (!sched.empty()) {
    for (DevBuf *b : {&ctx->dr_r, &ctx->dr_rs}) SDF_HIP(b->reserve(16));
    if (int rc = upload_all(ctx, D.st, {{ctx->dr_q, q.data(), q.size() * sizeof(sdf_minimizer)},
                                       {ctx->dr_r, r_own.data(), r_own.size() * sizeof(sdf_minimizer)},  // (empty under same_genome)
                                       {ctx->dr_rs, r_sorted.data(), r_sorted.size() * sizeof(sdf_minimizer)}}))
      return rc;
    D.d_q = (const sdf_minimizer *)ctx->dr_q.p;
    D.d_r = P.same_genome ? D.d_q : (const sdf_minimizer *)ctx->dr_r.p;
    D.d_rs = (const sdf_minimizer *)ctx->dr_rs.p;
    if (int rc = pair_rounds(D, sched)) return rc;
  }
  *stats = D.S;
  return pair_finish(ctx, D.out, out, cap, used);
}

extern "C" int sdf_search_pair(sdf_ctx *ctx, const sdf_minim_range *q_range, const sdf_minim_range *r_range, const sdf_search_pair_params *params,
                               sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats) {
  return pair_ranges(ctx, q_range, r_range, params, out, cap, used, stats, 0);
}

extern "C" int sdf_search_pair_wide(sdf_ctx *ctx, const sdf_minim_range *q_range, const sdf_minim_range *r_range,
                                    const sdf_search_pair_params *params, sdf_search_pair_hit *out, size_t cap, size_t *used,
                                    sdf_search_pair_stats *stats, size_t n_wide_max) {
  return pair_ranges(ctx, q_range, r_range, params, out, cap, used, stats, n_wide_max);
}

// ---- the resident search index: a range's minimizers and index once, for every pair that names the range ----

extern "C" int sdf_search_index_build(sdf_ctx *ctx, const sdf_minim_range *range, int k, int w, int separate_lowercase, sdf_search_index **out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!range || !out) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_index_build: invalid arguments");
  *out = nullptr;
  SDF_HIP(hipSetDevice(ctx->device));
  sdf_search_index *h = new sdf_search_index();
  h->ctx = ctx, h->pool_epoch = ctx->pool_epoch, h->range = *range, h->k = k, h->w = w, h->separate_lowercase = separate_lowercase != 0;
  auto fail = [&](int rc) {
    h->d_loc.release(), h->d_sorted.release();
    delete h;
    return rc;
  };
  // (the two calls check the range, k and w and refuse before their first launch)
  if (int rc = pair_minimizers(ctx, *range, k, w, separate_lowercase, false, h->loc, nullptr)) return fail(rc);
  if (int rc = pair_minimizers(ctx, *range, k, w, separate_lowercase, true, h->sorted, &h->threshold, &h->n_groups)) return fail(rc);
  // device copies of the handle's own, to the byte (never null: the device forms refuse a null pointer before they look at a count)
  hipError_t e = h->d_loc.reserve_exact(std::max<size_t>(h->loc.size() * sizeof(sdf_minimizer), 16));
  if (e == hipSuccess) e = h->d_sorted.reserve_exact(std::max<size_t>(h->sorted.size() * sizeof(sdf_minimizer), 16));
  if (e == hipSuccess && !h->loc.empty())
    e = hipMemcpyAsync(h->d_loc.p, h->loc.data(), h->loc.size() * sizeof(sdf_minimizer), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !h->sorted.empty())
    e = hipMemcpyAsync(h->d_sorted.p, h->sorted.data(), h->sorted.size() * sizeof(sdf_minimizer), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = std::string("sdf_search_index_build: ") + hipGetErrorString(e);
    return fail(e == hipErrorOutOfMemory ? SDF_ERR_NOMEM : SDF_ERR_HIP);
  }
  ctx->indexes.push_back(h);
  ctx->index_builds += 1;
  *out = h;
  return SDF_OK;
}

extern "C" int sdf_search_index_free(sdf_ctx *ctx, sdf_search_index *h) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!h) return SDF_OK;
  if (!index_live(ctx, h)) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_index_free: not a live handle of this context");
  SDF_HIP(hipSetDevice(ctx->device));
  ctx->indexes.erase(std::find(ctx->indexes.begin(), ctx->indexes.end(), h));
  h->d_loc.release(), h->d_sorted.release();
  delete h;
  return SDF_OK;
}

extern "C" int sdf_search_index_info(const sdf_ctx *ctx, const sdf_search_index *h, sdf_search_index_desc *info) {
  if (!ctx || !info || !index_live(ctx, h)) return SDF_ERR_INVALID;
  *info = sdf_search_index_desc{h->range,
                                h->k,
                                h->w,
                                h->separate_lowercase,
                                h->threshold,
                                (uint64_t)h->loc.size(),
                                (uint64_t)h->sorted.size(),
                                h->n_groups,
                                (uint32_t)(h->pool_epoch != ctx->pool_epoch),
                                (uint64_t)(h->d_loc.held_bytes() + h->d_sorted.held_bytes())};
  return SDF_OK;
}

extern "C" long long sdf_search_index_builds(const sdf_ctx *ctx) { return ctx ? ctx->index_builds : 0; }
extern "C" size_t sdf_search_index_live(const sdf_ctx *ctx) { return ctx ? ctx->indexes.size() : 0; }

// sdf_search_pair_indexed (n_wide_max == 0) and sdf_search_pair_indexed_wide: the rounds on `ctx`, the handles `owner`'s (the public
// calls name one context as both)
static int pair_handles(sdf_ctx *ctx, const sdf_ctx *owner, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                        sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats, size_t n_wide_max) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!used || !stats || !params || (cap && !out)) return refuse(ctx, SDF_ERR_INVALID, "sdf_search_pair_indexed: invalid arguments");
  std::vector<sdf_search_pair_hit> hits;
  sdf_search_pair_stats S;
  if (int rc = pair_handles_run(ctx, owner, q, r, params, n_wide_max, hits, &S)) return rc;
  *stats = S;
  return pair_finish(ctx, hits, out, cap, used);
}

extern "C" int sdf_search_pair_indexed(sdf_ctx *ctx, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                                       sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats) {
  return pair_handles(ctx, ctx, q, r, params, out, cap, used, stats, 0);
}

extern "C" int sdf_search_pair_indexed_wide(sdf_ctx *ctx, const sdf_search_index *q, const sdf_search_index *r,
                                            const sdf_search_pair_params *params, sdf_search_pair_hit *out, size_t cap, size_t *used,
                                            sdf_search_pair_stats *stats, size_t n_wide_max) {
  return pair_handles(ctx, ctx, q, r, params, out, cap, used, stats, n_wide_max);
}
