// The C ABI: search hits to seed records (include/sedef_hip.h states the contract; seed_records.hip holds the kernel, sdf_kernels.h
// the rule it shares with the `_host` form), and sdf_seeds_bucket_merge, the chain that `sedef seeds` runs: the records and their
// merge back to back on one stream.  The checks: sdf_entry.h (check_seed_scalars, check_seed, check_bucket_scalars).
#include <hip/hip_runtime.h>

#include "sdf_entry.h"

using namespace sdf;

namespace {
// the launch of a call on `st`, nothing read back (n >= 1, n_jobs >= 1)
int seed_launch(sdf_ctx *ctx, const sdf_search_pair_hit *d_hits, size_t n, const uint64_t *d_first, const sdf_seed_job *d_jobs, size_t n_jobs,
                sdf_seed_hit *d_out, hipStream_t st) {
  hipLaunchKernelGGL(seed_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_hits, (uint32_t)n, d_first, d_jobs, n_jobs, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 1;
  return SDF_OK;
}

// hits, first[] and the job table of a call in ONE buffer, in this order (24 n bytes keep first[] and the 64-bit field of a job
// on a multiple of eight); the copies are enqueued on `st`
struct SeedInputs {
  const sdf_search_pair_hit *hits;
  const uint64_t *first;
  const sdf_seed_job *jobs;
};
int seed_upload(sdf_ctx *ctx, hipStream_t st, const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs,
                size_t n_jobs, SeedInputs *d) {
  const size_t b_hits = n * sizeof(sdf_search_pair_hit), b_first = (n_jobs + 1) * sizeof(uint64_t), b_jobs = n_jobs * sizeof(sdf_seed_job);
  SDF_HIP(ctx->sd_in.reserve(b_hits + b_first + b_jobs));
  char *base = (char *)ctx->sd_in.p;
  SDF_HIP(hipMemcpyAsync(base, hits, b_hits, hipMemcpyHostToDevice, st));
  SDF_HIP(hipMemcpyAsync(base + b_hits, first, b_first, hipMemcpyHostToDevice, st));
  SDF_HIP(hipMemcpyAsync(base + b_hits + b_first, jobs, b_jobs, hipMemcpyHostToDevice, st));
  *d = SeedInputs{(const sdf_search_pair_hit *)base, (const uint64_t *)(base + b_hits), (const sdf_seed_job *)(base + b_hits + b_first)};
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_seed_records_host(const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs, size_t n_jobs,
                                     sdf_seed_hit *out) {
  std::string why;
  if (int rc = check_seed(hits, n, first, jobs, n_jobs, out, &why)) return rc;
  for (size_t t = 0; t < n; t++) out[t] = seed_record(hits[t], jobs[seed_job_of(first, n_jobs, t)]);
  return SDF_OK;
}

extern "C" int sdf_seed_records_device(sdf_ctx *ctx, const sdf_search_pair_hit *d_hits, size_t n, const uint64_t *d_first,
                                       const sdf_seed_job *d_jobs, size_t n_jobs, sdf_seed_hit *d_out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = "";
  if (int rc = check_seed_scalars(d_hits, n, d_first, d_jobs, n_jobs, d_out, &why)) return refuse(ctx, rc, std::string("sdf_seed_records_device: ") + why);
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  return seed_launch(ctx, d_hits, n, d_first, d_jobs, n_jobs, d_out, ctx->stream);
}

extern "C" int sdf_seed_records(sdf_ctx *ctx, const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs,
                                size_t n_jobs, sdf_seed_hit *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  std::string why;
  if (int rc = check_seed(hits, n, first, jobs, n_jobs, out, &why)) return refuse(ctx, rc, "sdf_seed_records: " + why);
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SeedInputs d;
  if (int rc = seed_upload(ctx, st, hits, n, first, jobs, n_jobs, &d)) return rc;
  SDF_HIP(ctx->sd_out.reserve(n * sizeof(sdf_seed_hit)));
  if (int rc = seed_launch(ctx, d.hits, n, d.first, d.jobs, n_jobs, (sdf_seed_hit *)ctx->sd_out.p, st)) return rc;
  SDF_HIP(hipMemcpyAsync(out, ctx->sd_out.p, n * sizeof(sdf_seed_hit), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// One upload, sdf_seed_records_device, sdf_bucket_merge_device behind it on the same stream, the two counts back, then the records.
extern "C" int sdf_seeds_bucket_merge(sdf_ctx *ctx, const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs,
                                      size_t n_jobs, const int32_t *chr_group, size_t n_chr, const int32_t *group_pair_order, size_t n_groups,
                                      const sdf_bucket_params *params, sdf_bucket_hit *out, size_t out_cap, size_t *n_out, size_t *n_dropped) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const std::string who = "sdf_seeds_bucket_merge: ";
  if (!n_dropped) return refuse(ctx, SDF_ERR_INVALID, who + "invalid arguments");
  std::string why;
  if (int rc = check_seed(hits, n, first, jobs, n_jobs, out, &why)) return refuse(ctx, rc, who + why);
  const char *w = "";
  if (int rc = check_bucket_scalars(hits, n, chr_group, n_chr, group_pair_order, n_groups, params, out, out_cap, n_out, &w))
    return refuse(ctx, rc, who + w);
  *n_out = 0, *n_dropped = 0;
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SeedInputs d;
  if (int rc = seed_upload(ctx, st, hits, n, first, jobs, n_jobs, &d)) return rc;
  const size_t b_chr = n_chr * sizeof(int32_t), b_pairs = n_groups * n_groups * sizeof(int32_t);
  SDF_HIP(ctx->sd_tab.reserve(b_chr + b_pairs));
  SDF_HIP(hipMemcpyAsync(ctx->sd_tab.p, chr_group, b_chr, hipMemcpyHostToDevice, st));
  SDF_HIP(hipMemcpyAsync((char *)ctx->sd_tab.p + b_chr, group_pair_order, b_pairs, hipMemcpyHostToDevice, st));
  SDF_HIP(ctx->sd_out.reserve(n * sizeof(sdf_seed_hit)));
  SDF_HIP(ctx->sd_merged.reserve(2 * sizeof(uint64_t) + n * sizeof(sdf_bucket_hit)));
  sdf_seed_hit *d_seeds = (sdf_seed_hit *)ctx->sd_out.p;
  uint64_t *d_n_out = (uint64_t *)ctx->sd_merged.p;
  sdf_bucket_hit *d_out = (sdf_bucket_hit *)(d_n_out + 2);
  if (int rc = sdf_seed_records_device(ctx, d.hits, n, d.first, d.jobs, n_jobs, d_seeds)) return rc;
  if (int rc = sdf_bucket_merge_device(ctx, d_seeds, n, (const int32_t *)ctx->sd_tab.p, n_chr, (const int32_t *)((char *)ctx->sd_tab.p + b_chr), n_groups,
                                       params, d_out, n, d_n_out))
    return rc;
  uint64_t counts[2] = {0, 0};
  SDF_HIP(hipMemcpyAsync(counts, d_n_out, sizeof counts, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  *n_dropped = (size_t)counts[1];
  if (counts[1] != 0) return SDF_OK;  // (the caller's to take elsewhere: nothing is copied back)
  if (counts[0] > n) return refuse(ctx, SDF_ERR_INVALID, who + "the device reports more records than seeds");
  if (counts[0]) SDF_HIP(hipMemcpyAsync(out, d_out, counts[0] * sizeof(sdf_bucket_hit), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  *n_out = (size_t)counts[0];
  return SDF_OK;
}
