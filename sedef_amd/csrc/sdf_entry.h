// The checks the entry points of the C ABI share (sdf_pool_api.hip, sdf_stats_api.hip, sdf_minim_api.hip, sdf_search_api.hip, sdf_filter_api.hip): is a range inside
// its pool, the tasks of the stats calls, and the tail of a call whose output the device counts first.
#pragma once
#include "sdf_ctx.h"

namespace sdf {
// a refusal: the call's error text and its code
inline int refuse(sdf_ctx *ctx, int code, std::string why) {
  ctx->err = std::move(why);
  return code;
}

// [off, off + len) lies inside [0, size) -- an empty range at `size` does -- without ever forming off + len (where that sum
// cannot wrap, a task's 63-bit offset and 31-bit length, this is off + len <= size: what batch_host and batch_pairs asked before)
inline bool in_range(uint64_t off, uint64_t len, uint64_t size) { return off <= size && len <= size - off; }
inline bool in_range(int64_t off, int64_t len, size_t size) { return off >= 0 && len >= 0 && in_range((uint64_t)off, (uint64_t)len, (uint64_t)size); }

// (the kernels that read the resident pool in aligned 16-byte units count them from its base)
inline bool pool_base_aligned(const sdf_ctx *ctx) { return ((uintptr_t)ctx->an_pool.p & 15) == 0; }

// The tasks of a stats call, in order; the first refusal is the call's.  noun: "columns" or "cuts".  resident: the tasks name
// ranges of the resident pool and may carry a strand bit per side in `reserved` (*any_rc: one does); else `reserved` is not
// looked at, and one sentence serves both ranges.
inline int check_stats_tasks(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, bool resident, const char *noun, size_t pool_bytes,
                             size_t cigar_words, bool *any_rc) {
  const uint32_t rc_bits = resident ? SDF_STATS_A_RC | SDF_STATS_B_RC : 0;
  auto refuse_task = [&](int code, size_t i, const char *why) { return refuse(ctx, code, "alignment " + std::to_string(i) + why); };
  *any_rc = false;
  for (size_t i = 0; i < n; i++) {
    const sdf_stats_task &t = tasks[i];
    if (resident && (t.reserved & ~rc_bits)) return refuse_task(SDF_ERR_UNSUPPORTED, i, ": unknown stats task flag");
    if (t.a_len > (1u << 24) || t.b_len > (1u << 24))
      return refuse(ctx, SDF_ERR_UNSUPPORTED, std::string("stats ") + noun + " implement sequences up to 16 Mb");
    if (!in_range(t.a_off, t.a_len, pool_bytes) || !in_range(t.b_off, t.b_len, pool_bytes))
      return refuse_task(SDF_ERR_INVALID, i, resident ? ": sequence range outside the resident pool (sdf_pool_upload / sdf_pool_append_fasta)"
                                                       : ": sequence or CIGAR range outside its pool");
    if (!in_range(t.cigar_off, t.n_cigar, cigar_words) || t.n_cigar >= (1u << 31))
      return refuse_task(SDF_ERR_INVALID, i, resident ? ": CIGAR range outside its pool" : ": sequence or CIGAR range outside its pool");
    *any_rc |= resident && t.reserved != 0;
  }
  return SDF_OK;
}

// The tail of a counted output, behind the launches that filled d_first[0 .. n] on `st`: first[0 .. n] back (a host form), or
// d_first[n] alone (first == nullptr: a device form), one wait, *used = the need, and SDF_ERR_CIGAR_OVERFLOW -- "<before>
// <need> <after>" -- when the need exceeds cap.
inline int counted_need(sdf_ctx *ctx, const uint64_t *d_first, size_t n, uint64_t *first, hipStream_t st, size_t cap, size_t *used,
                        const char *before, const char *after) {
  uint64_t last = 0;
  if (first) SDF_HIP(hipMemcpyAsync(first, d_first, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  else SDF_HIP(hipMemcpyAsync(&last, d_first + n, sizeof last, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  const uint64_t need = first ? first[n] : last;
  if (used) *used = (size_t)need;
  return need > cap ? refuse(ctx, SDF_ERR_CIGAR_OVERFLOW, before + std::to_string(need) + after) : SDF_OK;
}

// The found records of a search call (sdf_found_api.hip).  found_scalars: what every form checks of nf and of the bin entries
// the index may hold.  found_index: the launches that build the bin index of d_found[0, nf) on `st` into the context's fo_*
// buffers, at most `cap` entries; the need goes to fo_need and, when given, to *d_need; *F: the index as the kernels take it,
// with `d_visible` as its prefixes.  found_index_need: behind a wait on the stream, SDF_ERR_CIGAR_OVERFLOW when the need
// exceeded `cap`.
int found_scalars(size_t nf, size_t cap, const char **why);
int found_index(sdf_ctx *ctx, const sdf_search_found *d_found, size_t nf, size_t cap, uint64_t *d_need, const uint32_t *d_visible,
                hipStream_t st, FoundIndex *F);
int found_index_need(sdf_ctx *ctx, size_t cap);

// One window of initial_search on the host (sdf_search_api.hip, where the per-window forms of the stages live), for
// sdf_search_pair_host (sdf_driver_api.hip): include/sedef_hip.h states the steps.  pair_host_window runs window i against the
// whole of `found`, appends the records it keeps to it as it goes, and leaves the parse_hits survivors and the counters in W.
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
int pair_host_window(const PairHostArgs &A, size_t i, std::vector<sdf_search_found> &found, PairHostWindow &W);
}  // namespace sdf
