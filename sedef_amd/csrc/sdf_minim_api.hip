// The C ABI: winnowed minimizers of ranges of the resident pool and their index (minimizers.hip; include/sedef_hip.h).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "sdf_entry.h"

using namespace sdf;

extern "C" int sdf_minimizer_block(void) { return sdf::MINIM_BLOCK; }

// what every form checks of its scalars
static int minim_scalars(sdf_ctx *ctx, size_t n, int k, int w) {
  if (n > 0x3fffffffu || w < 1) {
    ctx->err = w < 1 ? "minimizers: w < 1" : "minimizers: more than 2^30 - 1 ranges";
    return SDF_ERR_INVALID;
  }
  if (k < 1 || k > 15 || w > sdf::MINIM_MAX_W) {
    ctx->err = "minimizers implement k 1..15 and w up to " + std::to_string(sdf::MINIM_MAX_W);
    return SDF_ERR_UNSUPPORTED;
  }
  return SDF_OK;
}
// ... and the host forms of their ranges.  blocks: what the launches will have (a range has at least one)
static int minim_ranges(sdf_ctx *ctx, const sdf_minim_range *r, size_t n, int k, bool *any_rc, uint64_t *blocks) {
  const size_t pool_bytes = ctx->pool_bytes;
  *any_rc = false;
  *blocks = 0;
  for (size_t i = 0; i < n; i++) {
    if (r[i].flags & ~SDF_MINIM_RC) return refuse(ctx, SDF_ERR_UNSUPPORTED, "minimizers: range " + std::to_string(i) + ": unknown flag");
    if (!in_range(r[i].off, r[i].len, pool_bytes))
      return refuse(ctx, SDF_ERR_INVALID, "minimizers: range " + std::to_string(i) + ": outside the resident pool");
    *any_rc |= (r[i].flags & SDF_MINIM_RC) != 0;
    *blocks += r[i].len >= k ? (uint64_t)((r[i].len - k) / sdf::MINIM_BLOCK + 1) : 1u;
  }
  if (*blocks > 0x3fffffffu) {
    ctx->err = "minimizers: more than 2^30 - 1 blocks of k-mer starts in one call";
    return SDF_ERR_UNSUPPORTED;
  }
  return SDF_OK;
}

// The five launches in front of the records: blocks per range and their scan (read back: *blocks), records per block and their
// scan, d_first.  Waits once, for the block count.
static int minim_count(sdf_ctx *ctx, const sdf_minim_range *d_ranges, size_t n, bool rev, int k, int w, int separate_lowercase,
                       uint64_t *d_first, uint64_t *blocks, hipStream_t st) {
  // (the kernels read aligned 16-byte units of the pool; no pool at all passes: it holds no range with a k-mer)
  if (!pool_base_aligned(ctx)) return refuse(ctx, SDF_ERR_INVALID, "minimizers: the pool's base is not 16-byte aligned");
  SDF_HIP(ctx->mz_plan.reserve(n * 4 + (n + 1) * 8 + 64));
  uint64_t *d_blk0 = (uint64_t *)ctx->mz_plan.p;
  uint32_t *d_blocks = (uint32_t *)(d_blk0 + n + 1);
  const long long pool_bytes = (long long)ctx->pool_bytes;
  hipLaunchKernelGGL(sdf::minim_blocks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_ranges, (int)n, pool_bytes, k, d_blocks);
  hipLaunchKernelGGL(sdf::stats_cuts_scan_kernel, dim3(1), dim3(1024), 0, st, d_blocks, (int)n, d_blk0);
  SDF_HIP(hipGetLastError());
  ctx->launches += 2;
  SDF_HIP(hipMemcpyAsync(blocks, d_blk0 + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  const uint64_t nb = *blocks;
  if (nb < n || nb > 0x3fffffffu) {
    ctx->err = "minimizers: more than 2^30 - 1 blocks of k-mer starts in one call";
    return SDF_ERR_UNSUPPORTED;
  }
  SDF_HIP(ctx->mz_counts.reserve(nb * 4 + (nb + 1) * 8 + 64));
  uint64_t *d_block_first = (uint64_t *)ctx->mz_counts.p;
  uint32_t *d_counts = (uint32_t *)(d_block_first + nb + 1);
  hipLaunchKernelGGL(rev ? sdf::minim_count_kernel<true> : sdf::minim_count_kernel<false>, dim3((unsigned)nb), dim3(64), 0, st, d_ranges,
                     (int)n, d_blk0, (const char *)ctx->an_pool.p, pool_bytes, k, w, separate_lowercase, d_counts);
  hipLaunchKernelGGL(sdf::stats_cuts_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, (int)nb, d_block_first);
  hipLaunchKernelGGL(sdf::minim_first_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, d_blk0, (int)n, d_block_first, d_first);
  SDF_HIP(hipGetLastError());
  ctx->launches += 3;
  return SDF_OK;
}
// the records (after minim_count on the same stream)
static int minim_emit(sdf_ctx *ctx, const sdf_minim_range *d_ranges, size_t n, bool rev, int k, int w, int separate_lowercase,
                      uint64_t blocks, sdf_minimizer *d_out, size_t cap, hipStream_t st) {
  const uint64_t *d_blk0 = (const uint64_t *)ctx->mz_plan.p, *d_block_first = (const uint64_t *)ctx->mz_counts.p;
  hipLaunchKernelGGL(rev ? sdf::minim_emit_kernel<true> : sdf::minim_emit_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, st, d_ranges,
                     (int)n, d_blk0, (const char *)ctx->an_pool.p, (long long)ctx->pool_bytes, k, w, separate_lowercase, d_block_first,
                     d_out, (uint64_t)cap);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}

extern "C" int sdf_pool_minimizers_device(sdf_ctx *ctx, const sdf_minim_range *d_ranges, size_t n, int any_rc, int k, int w,
                                          int separate_lowercase, uint64_t *d_first, sdf_minimizer *d_out, size_t cap, size_t *used,
                                          void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) {
    if (used) *used = 0;
    return SDF_OK;
  }
  if (!d_ranges || !d_first || (cap && !d_out)) {
    ctx->err = "sdf_pool_minimizers_device: invalid arguments";
    return SDF_ERR_INVALID;
  }
  if (int rc = minim_scalars(ctx, n, k, w)) return rc;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  uint64_t blocks = 0;
  if (int rc = minim_count(ctx, d_ranges, n, any_rc != 0, k, w, separate_lowercase, d_first, &blocks, st)) return rc;
  if (int rc = minim_emit(ctx, d_ranges, n, any_rc != 0, k, w, separate_lowercase, blocks, d_out, cap, st)) return rc;
  if (stream) return SDF_OK;
  return counted_need(ctx, d_first, n, nullptr, st, cap, used, "the ranges have ", " minimizers, more than cap");
}

// Both host forms up to the records in HBM: checks, upload, the launches.  SDF_OK: first[] and *used are filled and, when the
// records fit, *d_recs holds them (ctx->mz_out); SDF_ERR_CIGAR_OVERFLOW: first[] and *used only.
static int minim_host(sdf_ctx *ctx, const char *who, const sdf_minim_range *r, size_t n, int k, int w, int separate_lowercase,
                      uint64_t *first, const void *out, size_t cap, size_t *used, const sdf_minimizer **d_recs) {
  if (!r || !first || !used || (cap && !out)) {
    ctx->err = std::string(who) + ": invalid arguments";
    return SDF_ERR_INVALID;
  }
  if (int rc = minim_scalars(ctx, n, k, w)) return rc;
  bool any_rc = false;
  uint64_t blocks = 0;
  if (int rc = minim_ranges(ctx, r, n, k, &any_rc, &blocks)) return rc;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the pool's uploads were enqueued there)
  SDF_HIP(ctx->mz_ranges.reserve(n * sizeof(sdf_minim_range)));
  SDF_HIP(ctx->mz_first.reserve((n + 1) * sizeof(uint64_t)));
  const sdf_minim_range *d_ranges = (const sdf_minim_range *)ctx->mz_ranges.p;
  uint64_t *d_first = (uint64_t *)ctx->mz_first.p;
  SDF_HIP(hipMemcpyAsync(ctx->mz_ranges.p, r, n * sizeof(sdf_minim_range), hipMemcpyHostToDevice, st));
  if (int rc = minim_count(ctx, d_ranges, n, any_rc, k, w, separate_lowercase, d_first, &blocks, st)) return rc;
  if (int rc = counted_need(ctx, d_first, n, first, st, cap, used, "the ranges have ", " minimizers, more than cap")) return rc;
  const uint64_t need = first[n];
  SDF_HIP(ctx->mz_out.reserve((size_t)need * sizeof(sdf_minimizer) + 16));
  if (int rc = minim_emit(ctx, d_ranges, n, any_rc, k, w, separate_lowercase, blocks, (sdf_minimizer *)ctx->mz_out.p, (size_t)need, st)) return rc;
  *d_recs = (const sdf_minimizer *)ctx->mz_out.p;
  return SDF_OK;
}

extern "C" int sdf_pool_minimizers(sdf_ctx *ctx, const sdf_minim_range *r, size_t n, int k, int w, int separate_lowercase,
                                   uint64_t *first, sdf_minimizer *out, size_t cap, size_t *used) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) {
    if (used) *used = 0;
    if (first) first[0] = 0;
    return SDF_OK;
  }
  const sdf_minimizer *d_recs = nullptr;
  if (int rc = minim_host(ctx, "sdf_pool_minimizers", r, n, k, w, separate_lowercase, first, out, cap, used, &d_recs)) return rc;
  if (*used) SDF_HIP(hipMemcpyAsync(out, d_recs, *used * sizeof(sdf_minimizer), hipMemcpyDeviceToHost, ctx->stream));
  SDF_HIP(hipStreamSynchronize(ctx->stream));
  return SDF_OK;
}

extern "C" int sdf_pool_minimizer_index(sdf_ctx *ctx, const sdf_minim_range *r, size_t n, int k, int w, int separate_lowercase,
                                        uint64_t *first, sdf_minimizer *sorted, size_t cap, size_t *used, uint32_t *n_groups,
                                        uint32_t *threshold) {
  using namespace sdf;
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) {
    if (used) *used = 0;
    if (first) first[0] = 0;
    return SDF_OK;
  }
  if (!n_groups || !threshold) {
    ctx->err = "sdf_pool_minimizer_index: invalid arguments";
    return SDF_ERR_INVALID;
  }
  const sdf_minimizer *d_recs = nullptr;
  if (int rc = minim_host(ctx, "sdf_pool_minimizer_index", r, n, k, w, separate_lowercase, first, sorted, cap, used, &d_recs)) return rc;
  hipStream_t st = ctx->stream;
  const uint64_t m = *used;
  if (m == 0) {
    SDF_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) n_groups[i] = 0, threshold[i] = 0x80000000u;
    return SDF_OK;
  }
  if (m > 0x7fffffffu) {
    SDF_HIP(hipStreamSynchronize(st));
    ctx->err = "sdf_pool_minimizer_index: more than 2^31 - 1 minimizers in one call";
    return SDF_ERR_UNSUPPORTED;
  }
  int range_bits = 1;
  while (((size_t)1 << range_bits) < n) ++range_bits;
  const int key_bits = 32 + range_bits;
  // keys, sorted keys | places, sorted places | heads, ranks, starts (m + 1 each)
  SDF_HIP(ctx->mz_keys.reserve(2 * m * 8));
  SDF_HIP(ctx->mz_vals.reserve(2 * m * 4));
  SDF_HIP(ctx->mz_groups.reserve(3 * (m + 1) * 4));
  SDF_HIP(ctx->mz_sorted.reserve(m * sizeof(sdf_minimizer)));
  SDF_HIP(ctx->mz_res.reserve(2 * n * 4));
  unsigned long long *d_keys = (unsigned long long *)ctx->mz_keys.p, *d_keys2 = d_keys + m;
  uint32_t *d_vals = (uint32_t *)ctx->mz_vals.p, *d_vals2 = d_vals + m;
  uint32_t *d_flags = (uint32_t *)ctx->mz_groups.p, *d_gidx = d_flags + m + 1, *d_start = d_gidx + m + 1;
  sdf_minimizer *d_sorted = (sdf_minimizer *)ctx->mz_sorted.p;
  uint32_t *d_ng = (uint32_t *)ctx->mz_res.p, *d_thr = d_ng + n;
  size_t t_pairs = 0, t_keys = 0, t_scan = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_pairs, d_keys, d_keys2, d_vals, d_vals2, (int)m, 0, key_bits, st));
  SDF_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, t_keys, d_keys, d_keys2, (int)m, 0, key_bits, st));
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, d_flags, d_gidx, (int)(m + 1), st));
  SDF_HIP(ctx->mz_tmp.reserve(std::max({t_pairs, t_keys, t_scan}) + 256));
  const dim3 grid((unsigned)((m + 256) / 256)), block(256);  // (m + 1 lanes and more)
  hipLaunchKernelGGL(minim_keys_kernel, grid, block, 0, st, d_recs, (long long)m, d_keys, d_vals);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->mz_tmp.p, t_pairs, d_keys, d_keys2, d_vals, d_vals2, (int)m, 0, key_bits, st));
  hipLaunchKernelGGL(minim_heads_kernel, grid, block, 0, st, d_keys2, d_vals2, d_recs, (long long)m, d_sorted, d_flags);
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->mz_tmp.p, t_scan, d_flags, d_gidx, (int)(m + 1), st));
  hipLaunchKernelGGL(minim_starts_kernel, grid, block, 0, st, d_flags, d_gidx, (long long)m, d_start);
  SDF_HIP(hipGetLastError());
  ctx->launches += 3;
  uint32_t groups = 0;
  SDF_HIP(hipMemcpyAsync(&groups, d_gidx + m, 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(sorted, d_sorted, m * sizeof(sdf_minimizer), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  // the groups' size keys, in the first half of the key buffer (its keys are spent; the sorted ones, behind them, are read)
  hipLaunchKernelGGL(minim_sizes_kernel, dim3((groups + 255) / 256), block, 0, st, d_keys2, d_start, (long long)groups, d_keys);
  unsigned long long *d_size_keys = (unsigned long long *)ctx->mz_sorted.p;  // (the sorted records have left; 16 bytes a record: room for m keys)
  SDF_HIP(hipcub::DeviceRadixSort::SortKeys(ctx->mz_tmp.p, t_keys, d_keys, d_size_keys, (int)groups, 0, key_bits, st));
  hipLaunchKernelGGL(minim_threshold_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, st, d_size_keys, (long long)groups,
                     (const uint64_t *)ctx->mz_first.p, (int)n, d_ng, d_thr);
  SDF_HIP(hipGetLastError());
  ctx->launches += 2;
  SDF_HIP(hipMemcpyAsync(n_groups, d_ng, n * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(threshold, d_thr, n * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}
