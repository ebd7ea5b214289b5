// What the entry points of the C ABI share on the launch side (sdf_pool_api.hip, sdf_stats_api.hip, sdf_minim_api.hip and the
// search family's sdf_*_api.hip): a refusal, the tasks of the stats calls, the tail of a call whose output the device counts
// first, the bin index of the found records, and the uploads of a form that takes host arrays.  (in_range: sdf_internal.h;
// the search family's own checks and host rules: search_host.h.)
#pragma once
#include <initializer_list>

#include "sdf_ctx.h"

namespace sdf {
// a refusal: the call's error text and its code
inline int refuse(sdf_ctx *ctx, int code, std::string why) {
  ctx->err = std::move(why);
  return code;
}

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

// The regions and intervals of a coverage call (include/sedef_hip.h: sdf_pool_coverage / sdf_pool_coverage_host), in order; the
// first refusal is the call's, and *why its sentence.  Both forms ask this before they do anything.
inline int check_cover(const sdf_pool_range *regions, size_t n_regions, const sdf_cover_interval *iv, size_t n_iv, size_t pool_bytes,
                       const sdf_cover_counts *out, std::string *why) {
  const std::string who = "sdf_pool_coverage: ";
  if ((n_regions && (!regions || !out)) || (n_iv && !iv)) return *why = who + "invalid arguments", SDF_ERR_INVALID;
  if (n_regions > 0x7fffffffu || n_iv > 0x7fffffffu) return *why = who + "more than 2^31 - 1 regions or intervals in one call", SDF_ERR_UNSUPPORTED;
  for (size_t r = 0; r < n_regions; r++) {
    if (regions[r].reserved != 0) return *why = who + "region " + std::to_string(r) + ": reserved must be 0", SDF_ERR_UNSUPPORTED;
    if (!in_range(regions[r].off, (int64_t)regions[r].len, pool_bytes))
      return *why = who + "region " + std::to_string(r) + ": range outside the resident pool", SDF_ERR_INVALID;
  }
  for (size_t i = 0; i < n_iv; i++) {
    const sdf_cover_interval &v = iv[i];
    const auto refuse_iv = [&](int code, const char *what) { return *why = who + "interval " + std::to_string(i) + ": " + what, code; };
    if (v.reserved != 0) return refuse_iv(SDF_ERR_UNSUPPORTED, "reserved must be 0");
    if (v.set != 0 && v.set != 1) return refuse_iv(SDF_ERR_INVALID, "set must be 0 or 1");
    if (v.region < 0 || (size_t)v.region >= n_regions) return refuse_iv(SDF_ERR_INVALID, "region out of range");
    if (!in_range((int64_t)v.start, (int64_t)v.len, (size_t)regions[v.region].len)) return refuse_iv(SDF_ERR_INVALID, "not inside its region");
    if (v.partner < -1 || (v.partner >= 0 && (size_t)v.partner >= n_iv)) return refuse_iv(SDF_ERR_INVALID, "partner out of range");
  }
  return SDF_OK;
}

// What every form of the bucket family asks of its scalars (include/sedef_hip.h: sdf_bucket_merge), in order; the first refusal
// is the call's.  The pointers are the caller's arrays wherever they lie.
inline int check_bucket_scalars(const void *hits, size_t n, const void *chr_group, size_t n_chr, const void *group_pair_order, size_t n_groups,
                                const sdf_bucket_params *P, const void *out, size_t out_cap, const void *n_out, const char **why) {
  if (!P || !n_out) return *why = "invalid arguments", SDF_ERR_INVALID;
  if (P->nbins < 1) return *why = "nbins < 1", SDF_ERR_INVALID;
  if (P->merge_dist < 0 || P->max_extend < 0) return *why = "merge_dist or max_extend below 0", SDF_ERR_INVALID;
  if (!(P->extend_ratio >= 0)) return *why = "extend_ratio is negative or not a number", SDF_ERR_INVALID;
  if (n > ((size_t)1 << 30)) return *why = "more than 2^30 seed hits in one call", SDF_ERR_UNSUPPORTED;
  if (out_cap < n) return *why = "out_cap < n", SDF_ERR_INVALID;
  if (n == 0) return SDF_OK;
  if (!hits || !chr_group || !group_pair_order || !out) return *why = "invalid arguments", SDF_ERR_INVALID;
  if (n_chr < 1 || n_chr > ((size_t)1 << 19)) return *why = "n_chr outside 1 .. 2^19", SDF_ERR_INVALID;
  if (n_groups < 1 || n_groups > 4096) return *why = "n_groups outside 1 .. 4096", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and, where the arrays are the host's, of every table entry and record: recs[i] = hit i behind bucket_prepare
// (sdf_kernels.h: the record's own checks, Hit::extend, the ordered sides).
inline int check_bucket(const sdf_seed_hit *hits, size_t n, const int32_t *chr_group, size_t n_chr, const int32_t *group_pair_order,
                        size_t n_groups, const sdf_bucket_params *P, const void *out, size_t out_cap, const void *n_out,
                        std::vector<BucketRec> *recs, std::string *why) {
  const char *w = "";
  if (int rc = check_bucket_scalars(hits, n, chr_group, n_chr, group_pair_order, n_groups, P, out, out_cap, n_out, &w)) return *why = w, rc;
  recs->resize(n);
  if (n == 0) return SDF_OK;
  for (size_t c = 0; c < n_chr; c++)
    if (chr_group[c] < 0 || (size_t)chr_group[c] >= n_groups) return *why = "chromosome " + std::to_string(c) + ": group out of range", SDF_ERR_INVALID;
  for (size_t g = 0; g < n_groups * n_groups; g++)
    if (group_pair_order[g] < 0 || (size_t)group_pair_order[g] >= n_groups * n_groups)
      return *why = "group_pair_order entry " + std::to_string(g) + " out of range", SDF_ERR_INVALID;
  for (size_t i = 0; i < n; i++) {
    (*recs)[i] = bucket_prepare(hits[i], chr_group, (int32_t)n_chr, group_pair_order, (int32_t)n_groups, P->extend_ratio, P->max_extend, P->merge_dist);
    if ((*recs)[i].flags & kBucketBad)
      return *why = "seed hit " + std::to_string(i) + ": an id, a coordinate, a flag or its extension is outside what the call takes", SDF_ERR_INVALID;
  }
  return SDF_OK;
}

// What every form of sdf_seed_records asks (include/sedef_hip.h), in order; the first refusal is the call's.  The pointers are the
// caller's arrays wherever they lie ...
inline int check_seed_scalars(const void *hits, size_t n, const void *first, const void *jobs, size_t n_jobs, const void *out, const char **why) {
  if (n > ((size_t)1 << 30)) return *why = "more than 2^30 hits in one call", SDF_ERR_UNSUPPORTED;
  if (n > 0 && (!hits || !first || !jobs || !out)) return *why = "invalid arguments", SDF_ERR_INVALID;
  if (n > 0 && n_jobs == 0) return *why = "first[n_jobs] != n", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and, where first[] and the job table are the host's, of every entry (with n == 0 too, where they are given).
inline int check_seed(const void *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs, size_t n_jobs, const void *out, std::string *why) {
  const char *w = "";
  if (int rc = check_seed_scalars(hits, n, first, jobs, n_jobs, out, &w)) return *why = w, rc;
  for (size_t j = 0; jobs && j < n_jobs; j++)
    if (jobs[j].reserved != 0 || (jobs[j].flags & ~SDF_SEED_RC))
      return *why = "job " + std::to_string(j) + ": reserved must be 0, flags SDF_SEED_RC or 0", SDF_ERR_UNSUPPORTED;
  if (!first) return SDF_OK;  // (n == 0 and no table)
  if (first[0] != 0) return *why = "first[0] != 0", SDF_ERR_INVALID;
  for (size_t j = 0; j < n_jobs; j++)
    if (first[j + 1] < first[j]) return *why = "first[] decreases at job " + std::to_string(j), SDF_ERR_INVALID;
  if (first[n_jobs] != n) return *why = "first[n_jobs] != n", SDF_ERR_INVALID;
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

// Two handles as a pair (sdf_driver_api.hip), for the single-pair calls and for the lanes (sdf_lanes_api.hip).  `owner` holds
// the handles; the rounds run on `ctx`, the owner itself or a lane that views its pool.  pair_handles_valid: what
// sdf_search_pair_indexed asks of the handles against the owner and the parameters (SDF_ERR_INVALID); pair_handles_ranges: behind
// it, sdf_search_pair's refusals on the handles' ranges and on n_wide_max, with their codes; neither reads a handle that is not
// live, neither launches.  pair_handles_run: both checks, then the rounds; the pair's hits to `hits`.
int pair_handles_valid(const sdf_ctx *owner, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                       const char **why);
int pair_handles_ranges(size_t pool_bytes, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                        size_t n_wide_max, const char **why);
int pair_handles_run(sdf_ctx *ctx, const sdf_ctx *owner, const sdf_search_index *q, const sdf_search_index *r,
                     const sdf_search_pair_params *params, size_t n_wide_max, std::vector<sdf_search_pair_hit> &hits,
                     sdf_search_pair_stats *stats);

// The uploads of a form that takes host arrays: every buffer reserved and its copy enqueued on `st`, in order; an entry of no
// bytes is skipped (its buffer stays as it is).
struct Upload {
  DevBuf &buf;
  const void *src;
  size_t bytes;
};
inline int upload_all(sdf_ctx *ctx, hipStream_t st, std::initializer_list<Upload> uploads) {
  for (const Upload &u : uploads) {
    if (!u.bytes) continue;
    SDF_HIP(u.buf.reserve(u.bytes));
    SDF_HIP(hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, st));
  }
  return SDF_OK;
}
}  // namespace sdf
