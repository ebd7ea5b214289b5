// The C ABI: search against the SDs already found (search_found.hip; include/sedef_hip.h states the rules) -- the launches of
// the bin index of the found records, which sdf_search_windows_found* (sdf_search_api.hip) reads too, and the device and
// uploading forms of is_overlap for every rolled interval.  sdf_search_overlap_host, sdf_search_found_entries and the
// checks: search_host.hip.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "sdf_entry.h"
#include "search_host.h"

using namespace sdf;

namespace sdf {
int found_scalars(size_t nf, size_t cap, const char **why) {
  if (nf > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 found records in one call", SDF_ERR_UNSUPPORTED;
  if (cap > 0x7fffffffu) return *why = "search found: more than 2^31 - 1 bin entries in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

int found_index(sdf_ctx *ctx, const sdf_search_found *d_found, size_t nf, size_t cap, uint64_t *d_need, const uint32_t *d_visible,
                hipStream_t st, FoundIndex *F) {
  constexpr size_t kWords = (size_t)FOUND_BINS + 1;  // the last count stays 0: its start is the list's entries
  SDF_HIP(ctx->fo_need.reserve(8));
  *F = FoundIndex{d_found, nullptr, nullptr, d_visible, 0, (uint32_t)nf};
  if (nf == 0) {
    SDF_HIP(hipMemsetAsync(ctx->fo_need.p, 0, 8, st));
    if (d_need) SDF_HIP(hipMemsetAsync(d_need, 0, 8, st));
    return SDF_OK;
  }
  SDF_HIP(ctx->fo_counts.reserve(kWords * 8));
  SDF_HIP(ctx->fo_start.reserve(kWords * 8));
  SDF_HIP(ctx->fo_ent.reserve((cap ? cap : 1) * 4));
  unsigned long long *d_counts = (unsigned long long *)ctx->fo_counts.p, *d_start = (unsigned long long *)ctx->fo_start.p;
  size_t t_scan = 0;
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, d_counts, d_start, (int)kWords, st));
  SDF_HIP(ctx->fo_tmp.reserve(t_scan + 256));
  SDF_HIP(hipMemsetAsync(d_counts, 0, kWords * 8, st));
  const dim3 grid((unsigned)((nf + 255) / 256)), block(256);
  hipLaunchKernelGGL(found_count_kernel, grid, block, 0, st, d_found, (int)nf, d_counts);
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->fo_tmp.p, t_scan, d_counts, d_start, (int)kWords, st));
  hipLaunchKernelGGL(found_fill_kernel, grid, block, 0, st, d_found, (int)nf, (const unsigned long long *)d_start, d_counts,
                     (uint32_t *)ctx->fo_ent.p, (unsigned long long)cap, (unsigned long long *)ctx->fo_need.p);
  SDF_HIP(hipGetLastError());
  ctx->launches += 3;
  if (d_need) SDF_HIP(hipMemcpyAsync(d_need, ctx->fo_need.p, 8, hipMemcpyDeviceToDevice, st));
  F->start = d_start, F->entries = (const uint32_t *)ctx->fo_ent.p, F->cap = cap;
  return SDF_OK;
}

int found_index_need(sdf_ctx *ctx, size_t cap) {
  uint64_t need = 0;
  SDF_HIP(hipMemcpy(&need, ctx->fo_need.p, 8, hipMemcpyDeviceToHost));
  return need > cap ? refuse(ctx, SDF_ERR_CIGAR_OVERFLOW,
                             "the found records have " + std::to_string(need) + " bin entries, more than found_entries_cap")
                    : SDF_OK;
}
}  // namespace sdf

namespace {
int overlap_launch(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const uint64_t *d_first, const sdf_search_roll_rec *d_rolls, size_t n,
                   const FoundIndex &F, int32_t init_len, int32_t min_read_size, uint32_t *d_out, sdf_filter_task *d_tasks, hipStream_t st) {
  if (F.nf == 0) {  // no record: every verdict is 0, and no task changes
    SDF_HIP(hipMemsetAsync(d_out, 0, n * 4, st));
    return SDF_OK;
  }
  hipLaunchKernelGGL(search_overlap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_q, (int)nq, d_first, d_rolls, (int)n, F,
                     (int)init_len, (int)min_read_size, d_out, d_tasks);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_search_overlap_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const uint64_t *d_first,
                                         const sdf_search_roll_rec *d_rolls, size_t n_max, const sdf_search_found *d_found, size_t nf,
                                         size_t found_entries_cap, uint64_t *d_found_entries, const uint32_t *d_visible_iv, int32_t init_len,
                                         int32_t min_read_size, uint32_t *d_out, sdf_filter_task *d_filter_tasks, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0 || n_max == 0) return SDF_OK;
  if (!d_q || !d_first || !d_rolls || !d_visible_iv || !d_out || (nf && !d_found))
    return refuse(ctx, SDF_ERR_INVALID, "sdf_search_overlap_device: invalid arguments");
  const char *why = nullptr;
  if (int rc = overlap_scalars(nq, n_max, init_len, min_read_size, &why)) return refuse(ctx, rc, why);
  if (int rc = found_scalars(nf, found_entries_cap, &why)) return refuse(ctx, rc, why);
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  FoundIndex F{};
  if (int rc = found_index(ctx, d_found, nf, found_entries_cap, d_found_entries, d_visible_iv, st, &F)) return rc;
  if (int rc = overlap_launch(ctx, d_q, nq, d_first, d_rolls, n_max, F, init_len, min_read_size, d_out, d_filter_tasks, st)) return rc;
  if (stream) return SDF_OK;
  SDF_HIP(hipStreamSynchronize(st));
  return found_index_need(ctx, found_entries_cap);
}

extern "C" int sdf_search_overlap(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const uint64_t *first, const sdf_search_roll_rec *rolls,
                                  const sdf_search_found *found, size_t nf, const uint32_t *visible_iv, int32_t init_len,
                                  int32_t min_read_size, uint32_t *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (nq == 0) return SDF_OK;
  const char *why = nullptr;
  uint64_t entries = 0;
  if (int rc = overlap_arrays(q, nq, first, rolls, found, nf, visible_iv, init_len, min_read_size, out, &entries, &why))
    return refuse(ctx, rc, why);
  const size_t n = (size_t)first[nq];
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_all(ctx, st, {{ctx->fo_q, q, nq * sizeof(sdf_minimizer)}, {ctx->fo_first, first, (nq + 1) * 8},
                                   {ctx->fo_rolls, rolls, n * sizeof(sdf_search_roll_rec)}, {ctx->fo_found, found, nf * sizeof(sdf_search_found)},
                                   {ctx->fo_vis, visible_iv, n * 4}}))
    return rc;
  SDF_HIP(ctx->fo_out.reserve(n * 4));
  FoundIndex F{};
  if (int rc = found_index(ctx, (const sdf_search_found *)ctx->fo_found.p, nf, (size_t)entries, nullptr, (const uint32_t *)ctx->fo_vis.p, st, &F))
    return rc;
  if (int rc = overlap_launch(ctx, (const sdf_minimizer *)ctx->fo_q.p, nq, (const uint64_t *)ctx->fo_first.p,
                              (const sdf_search_roll_rec *)ctx->fo_rolls.p, n, F, init_len, min_read_size, (uint32_t *)ctx->fo_out.p, nullptr, st))
    return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->fo_out.p, n * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}
