// The C ABI, `stats generate`: the columns of alignments and their cuts at assembly gaps (stats_cols.hip, stats_cuts.hip).
#include <hip/hip_runtime.h>

#include "sdf_entry.h"

using namespace sdf;

// ---- per-alignment columns of `stats generate` (reference: src/stats_main.cc:228-270) -------------------
// the two launches of the stats kernels; rev: some task carries a strand bit (stats_cols.hip: the <true> kernels)
static int stats_launch(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, const char *d_seq_pool, const uint32_t *d_cigar_pool,
                        sdf_stats_cols *d_out, void *stream, bool rev) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n >= ((size_t)1 << 31) || (n && (!d_tasks || !d_out))) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  // the list for the segments of long alignments (stats_cols.hip): 2^18 segments of 512 runs; an alignment that finds it
  // full is counted by its own wavefront
  const unsigned kItems = (unsigned)ctx->cfg.stats_items;
  SDF_HIP(ctx->st_items.reserve((size_t)kItems * sizeof(sdf::StatsItem) + 64));
  unsigned *d_counter = reinterpret_cast<unsigned *>((char *)ctx->st_items.p + (size_t)kItems * sizeof(sdf::StatsItem));
  SDF_HIP(hipMemsetAsync(d_counter, 0, sizeof(unsigned), st));
  const unsigned group_max = ctx->cfg.stats_group_max >= 0 ? (unsigned)ctx->cfg.stats_group_max : sdf::STATS_GROUP_MAX;
  static_assert(sdf::STATS_WAVES == 4, "a workgroup is the four wavefronts of four consecutive alignments");
  hipLaunchKernelGGL(rev ? sdf::stats_columns_kernel<true> : sdf::stats_columns_kernel<false>,
                     dim3((unsigned)((n + sdf::STATS_WAVES - 1) / sdf::STATS_WAVES)),
                     dim3(64 * sdf::STATS_WAVES), 0, st, d_tasks, (int)n, d_seq_pool, d_cigar_pool, d_out,
                     (sdf::StatsItem *)ctx->st_items.p, d_counter, kItems, group_max);
  hipLaunchKernelGGL(rev ? sdf::stats_segments_kernel<true> : sdf::stats_segments_kernel<false>, dim3(2048), dim3(64 * sdf::STATS_WAVES), 0, st,
                     (const sdf::StatsItem *)ctx->st_items.p, d_counter, kItems, d_seq_pool, d_cigar_pool, d_out);
  SDF_HIP(hipGetLastError());
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

extern "C" int sdf_stats_columns_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, const char *d_seq_pool,
                                        const uint32_t *d_cigar_pool, sdf_stats_cols *d_out, void *stream) {
  return stats_launch(ctx, d_tasks, n, d_seq_pool, d_cigar_pool, d_out, stream, false);
}

// ... on the resident pool, by range and strand (include/sedef_hip.h)
extern "C" int sdf_stats_columns_pairs_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, int any_rc,
                                              const uint32_t *d_cigar_pool, sdf_stats_cols *d_out, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  return stats_launch(ctx, d_tasks, n, (const char *)ctx->an_pool.p, d_cigar_pool, d_out, stream, any_rc != 0);
}

// The host forms: tasks and runs from the host, records back.  resident: the tasks name ranges of the resident pool and may
// carry a strand bit per side in `reserved` (else: of seq_pool, uploaded here behind the checks -- nothing leaves the
// caller's memory for a call that is refused -- and `reserved` is not looked at).
static int stats_host(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, bool resident, const char *seq_pool, size_t pool_bytes,
                      const uint32_t *cigar_pool, size_t cigar_words, sdf_stats_cols *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n >= ((size_t)1 << 31) || (n && (!tasks || !out)) || (!seq_pool && !resident && pool_bytes) || (!cigar_pool && cigar_words)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  bool any_rc = false;  // (the one scan of the tasks: a call without a reversed side gets the kernels as they were)
  if (int rc = check_stats_tasks(ctx, tasks, n, resident, "columns", pool_bytes, cigar_words, &any_rc)) return rc;
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the pool's uploads were enqueued there)
  SDF_HIP(ctx->st_tasks.reserve(n * sizeof(sdf_stats_task)));
  if (!resident) SDF_HIP(ctx->st_pool.reserve(pool_bytes + 16));
  SDF_HIP(ctx->st_cig.reserve(cigar_words * 4 + 16));
  SDF_HIP(ctx->st_out.reserve(n * sizeof(sdf_stats_cols)));
  SDF_HIP(hipMemcpyAsync(ctx->st_tasks.p, tasks, n * sizeof(sdf_stats_task), hipMemcpyHostToDevice, st));
  if (!resident && pool_bytes) SDF_HIP(hipMemcpyAsync(ctx->st_pool.p, seq_pool, pool_bytes, hipMemcpyHostToDevice, st));
  if (cigar_words) SDF_HIP(hipMemcpyAsync(ctx->st_cig.p, cigar_pool, cigar_words * 4, hipMemcpyHostToDevice, st));
  // (long alignments are cut into segments on the device: stats_cols.hip)
  const int rc = stats_launch(ctx, (const sdf_stats_task *)ctx->st_tasks.p, n, (const char *)(resident ? ctx->an_pool.p : ctx->st_pool.p),
                              (const uint32_t *)ctx->st_cig.p, (sdf_stats_cols *)ctx->st_out.p, st, any_rc);
  if (rc != SDF_OK) return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->st_out.p, n * sizeof(sdf_stats_cols), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  static_assert(sizeof(sdf_stats_cols) == 16 * sizeof(int32_t), "sdf_stats_cols is sixteen counters");
  for (size_t i = 0; i < n; i++)
    if (out[i].flags) {
      ctx->err = "alignment " + std::to_string(i) + ": the CIGAR does not fit its sequences";
      return SDF_ERR_INVALID;
    }
  return SDF_OK;
}

extern "C" int sdf_stats_columns_batch(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const char *seq_pool,
                                       size_t pool_bytes, const uint32_t *cigar_pool, size_t cigar_words,
                                       sdf_stats_cols *out) {
  return stats_host(ctx, tasks, n, false, seq_pool, pool_bytes, cigar_pool, cigar_words, out);
}

extern "C" int sdf_stats_columns_pairs(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const uint32_t *cigar_pool,
                                       size_t cigar_words, sdf_stats_cols *out) {
  return stats_host(ctx, tasks, n, true, nullptr, ctx ? ctx->pool_bytes : 0, cigar_pool, cigar_words, out);
}

// ---- the cuts of `stats generate` on the resident pool (stats_cuts.hip; include/sedef_hip.h) -------------------
static int cuts_scores(sdf_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, sdf::CutsScores &sc) {
  if (std::abs(match) > 63 || std::abs(mismatch) > 63 || std::abs(gap_open) > 63 || std::abs(gap_extend) > 63 ||
      std::abs(gap_open) + std::abs(gap_extend) > 63) {
    ctx->err = "stats cuts implement |match|, |mismatch| <= 63 and |gap_open| + |gap_extend| <= 63";
    return SDF_ERR_UNSUPPORTED;
  }
  sc = sdf::CutsScores{match, mismatch, gap_open, gap_extend};
  return SDF_OK;
}

// launches 1 and 2: the alignments' count words and first[]
static int cuts_count(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, bool rev, const uint32_t *d_cigar_pool, uint64_t *d_first,
                      hipStream_t st) {
  SDF_HIP(ctx->sc_counts.reserve(n * 12 + 64));
  uint32_t *d_counts = (uint32_t *)ctx->sc_counts.p;
  int32_t *d_whole = (int32_t *)(d_counts + n);
  const dim3 grid((unsigned)((n + sdf::STATS_WAVES - 1) / sdf::STATS_WAVES)), block(64 * sdf::STATS_WAVES);
  hipLaunchKernelGGL(rev ? sdf::stats_cuts_count_kernel<true> : sdf::stats_cuts_count_kernel<false>, grid, block, 0, st, d_tasks, (int)n,
                     (const char *)ctx->an_pool.p, d_cigar_pool, d_counts, d_whole);
  hipLaunchKernelGGL(sdf::stats_cuts_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, (int)n, d_first);
  SDF_HIP(hipGetLastError());
  ctx->launches += 2;
  return SDF_OK;
}
// launch 3: the records (after cuts_count on the same stream)
static int cuts_emit(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, bool rev, const uint32_t *d_cigar_pool, const sdf::CutsScores &sc,
                     const uint64_t *d_first, sdf_stats_piece *d_pieces, size_t cap, hipStream_t st) {
  const uint32_t *d_counts = (const uint32_t *)ctx->sc_counts.p;
  const int32_t *d_whole = (const int32_t *)(d_counts + n);
  const dim3 grid((unsigned)((n + sdf::STATS_WAVES - 1) / sdf::STATS_WAVES)), block(64 * sdf::STATS_WAVES);
  hipLaunchKernelGGL(rev ? sdf::stats_cuts_emit_kernel<true> : sdf::stats_cuts_emit_kernel<false>, grid, block, 0, st, d_tasks, (int)n,
                     (const char *)ctx->an_pool.p, d_cigar_pool, sc, d_counts, d_whole, d_first, d_pieces, (uint64_t)cap);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}

extern "C" int sdf_stats_cuts_pairs_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, int any_rc, const uint32_t *d_cigar_pool,
                                           int match, int mismatch, int gap_open, int gap_extend, uint64_t *d_first,
                                           sdf_stats_piece *d_pieces, size_t pieces_cap, size_t *pieces_used, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n >= ((size_t)1 << 31) || !d_first || (n && !d_tasks) || (pieces_cap && !d_pieces)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  sdf::CutsScores sc;
  if (int rc = cuts_scores(ctx, match, mismatch, gap_open, gap_extend, sc)) return rc;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (n == 0) {
    SDF_HIP(hipMemsetAsync(d_first, 0, sizeof(uint64_t), st));
    if (!stream) SDF_HIP(hipStreamSynchronize(st));
    if (pieces_used) *pieces_used = 0;
    return SDF_OK;
  }
  if (int rc = cuts_count(ctx, d_tasks, n, any_rc != 0, d_cigar_pool, d_first, st)) return rc;
  if (int rc = cuts_emit(ctx, d_tasks, n, any_rc != 0, d_cigar_pool, sc, d_first, d_pieces, pieces_cap, st)) return rc;
  if (stream) return SDF_OK;
  return counted_need(ctx, d_first, n, nullptr, st, pieces_cap, pieces_used, "the batch cuts into ", " pieces, more than pieces_cap");
}

extern "C" int sdf_stats_cuts_pairs(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const uint32_t *cigar_pool, size_t cigar_words,
                                    int match, int mismatch, int gap_open, int gap_extend, uint64_t *first, sdf_stats_piece *pieces,
                                    size_t pieces_cap, size_t *pieces_used) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n >= ((size_t)1 << 31) || !first || !pieces_used || (n && !tasks) || (pieces_cap && !pieces) || (!cigar_pool && cigar_words)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  sdf::CutsScores sc;
  if (int rc = cuts_scores(ctx, match, mismatch, gap_open, gap_extend, sc)) return rc;
  bool any_rc = false;
  if (int rc = check_stats_tasks(ctx, tasks, n, true, "cuts", ctx->pool_bytes, cigar_words, &any_rc)) return rc;
  *pieces_used = 0;
  first[0] = 0;
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the pool's uploads were enqueued there)
  SDF_HIP(ctx->sc_tasks.reserve(n * sizeof(sdf_stats_task)));
  SDF_HIP(ctx->sc_cig.reserve(cigar_words * 4 + 16));
  SDF_HIP(ctx->sc_first.reserve((n + 1) * sizeof(uint64_t)));
  const sdf_stats_task *d_tasks = (const sdf_stats_task *)ctx->sc_tasks.p;
  const uint32_t *d_cig = (const uint32_t *)ctx->sc_cig.p;
  uint64_t *d_first = (uint64_t *)ctx->sc_first.p;
  SDF_HIP(hipMemcpyAsync(ctx->sc_tasks.p, tasks, n * sizeof(sdf_stats_task), hipMemcpyHostToDevice, st));
  if (cigar_words) SDF_HIP(hipMemcpyAsync(ctx->sc_cig.p, cigar_pool, cigar_words * 4, hipMemcpyHostToDevice, st));
  if (int rc = cuts_count(ctx, d_tasks, n, any_rc, d_cig, d_first, st)) return rc;
  if (int rc = counted_need(ctx, d_first, n, first, st, pieces_cap, pieces_used, "the batch cuts into ", " pieces, more than pieces_cap")) return rc;
  const uint64_t need = first[n];
  SDF_HIP(ctx->sc_out.reserve((size_t)need * sizeof(sdf_stats_piece)));
  if (int rc = cuts_emit(ctx, d_tasks, n, any_rc, d_cig, sc, d_first, (sdf_stats_piece *)ctx->sc_out.p, (size_t)need, st)) return rc;
  SDF_HIP(hipMemcpyAsync(pieces, ctx->sc_out.p, (size_t)need * sizeof(sdf_stats_piece), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  static_assert(sizeof(sdf_stats_piece) == 32, "sdf_stats_piece: two records per 64-byte line");
  for (size_t i = 0; i < n; i++)
    if (pieces[first[i]].flags) {
      ctx->err = "alignment " + std::to_string(i) + ": the CIGAR does not fit its sequences";
      return SDF_ERR_INVALID;
    }
  return SDF_OK;
}
