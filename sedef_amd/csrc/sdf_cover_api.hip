// The C ABI: coverage of ranges of the resident pool by two interval sets (include/sedef_hip.h states the contract;
// pool_cover.hip holds the kernels) -- the device form and the `_host` form, over the one check (sdf_entry.h: check_cover) and
// the one layout of the bitmaps.
#include <hip/hip_runtime.h>

#include "sdf_entry.h"

using namespace sdf;

namespace {
// The records the kernels take; the totals: words of a set's bitmaps, wavefronts of the count launch, pieces of the intervals.
struct CoverLayout {
  std::vector<CoverRegion> regions;
  std::vector<CoverIv> iv;
  long long set_words = 0, n_waves = 0, n_pieces = 0;
};
int cover_layout(const sdf_pool_range *regions, size_t n_regions, const sdf_cover_interval *iv, size_t n_iv, CoverLayout &L, std::string *why) {
  L.regions.resize(n_regions);
  L.iv.resize(n_iv);
  for (size_t r = 0; r < n_regions; r++) {
    const long long words = ((long long)regions[r].len + 31) >> 5;
    L.regions[r] = CoverRegion{regions[r].off, L.set_words, L.n_waves, regions[r].len, 0};
    L.set_words += words;
    L.n_waves += (words + 63) >> 6;
  }
  for (size_t i = 0; i < n_iv; i++) {
    const CoverRegion &R = L.regions[(size_t)iv[i].region];
    L.iv[i] = CoverIv{R.off + iv[i].start, 32 * R.word0 + iv[i].start, iv[i].len, iv[i].set, iv[i].partner, (int32_t)L.n_pieces};
    L.n_pieces += ((long long)iv[i].len + kCoverPieceBytes - 1) / kCoverPieceBytes;
    if (L.n_pieces > 0x7fffff00ll) return *why = "sdf_pool_coverage: more than 2^31 pieces of intervals in one call", SDF_ERR_UNSUPPORTED;
  }
  // (a launch's grid is a wavefront per four: 2^33 wavefronts are 2^44 bases)
  if (L.n_waves > 0x1fffffff00ll) return *why = "sdf_pool_coverage: more than 2^44 bases of regions in one call", SDF_ERR_UNSUPPORTED;
  return SDF_OK;
}

void cover_painted_all(const sdf_cover_interval *iv, size_t n_iv, const int32_t *upper, int32_t min_upper, uint8_t *painted) {
  for (size_t i = 0; i < n_iv; i++)
    painted[i] = cover_painted(iv[i].partner, upper[i], iv[i].partner < 0 ? 0 : upper[iv[i].partner], min_upper);
}
}  // namespace

extern "C" int sdf_pool_coverage(sdf_ctx *ctx, const sdf_pool_range *regions, size_t n_regions, const sdf_cover_interval *iv, size_t n_iv,
                                 int32_t min_upper, sdf_cover_counts *out, int32_t *iv_upper, uint8_t *iv_painted) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  std::string why;
  if (int rc = check_cover(regions, n_regions, iv, n_iv, ctx->pool_bytes, out, &why)) return refuse(ctx, rc, why);
  if (n_regions == 0) return SDF_OK;  // (and no interval: each would name a region)
  CoverLayout L;
  if (int rc = cover_layout(regions, n_regions, iv, n_iv, L, &why)) return refuse(ctx, rc, why);
  memset(out, 0, n_regions * sizeof(sdf_cover_counts));
  std::vector<int32_t> upper(n_iv, 0);
  const auto finish = [&]() {
    if (iv_upper && n_iv) memcpy(iv_upper, upper.data(), n_iv * sizeof(int32_t));
    if (iv_painted) cover_painted_all(iv, n_iv, upper.data(), min_upper, iv_painted);
    return SDF_OK;
  };
  if (L.set_words == 0) return finish();  // (no base in any region: every interval is empty)
  // (the count launch reads aligned slots: those of a region at the pool's base start there, those of one at its end lie in the
  // 64 bytes behind every pool allocation)
  if (!pool_base_aligned(ctx) || ctx->an_pool.cap < ctx->pool_bytes + 16)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_pool_coverage: the pool's base is not 16-byte aligned, or nothing is allocated behind its last character");
  SDF_HIP(hipSetDevice(ctx->device));
  const size_t bits_bytes = 2 * (size_t)L.set_words * sizeof(uint32_t);
  const size_t rec_bytes = n_regions * (sizeof(CoverRegion) + sizeof(sdf_cover_counts)) + n_iv * (sizeof(CoverIv) + sizeof(int32_t));
  if (bits_bytes > ctx->cv_bits.cap) {  // (the bitmaps grow: beside what the device holds)
    size_t free_b = 0, total_b = 0;
    SDF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bits_bytes + 2 * rec_bytes + ((size_t)64 << 20) > free_b)
      return refuse(ctx, SDF_ERR_INVALID, "sdf_pool_coverage: the bitmaps do not fit the device's free memory");
  }
  hipStream_t st = ctx->stream;  // (the pool's uploads were enqueued there)
  for (DevBuf *b : {&ctx->cv_regions, &ctx->cv_iv, &ctx->cv_upper, &ctx->cv_out, &ctx->cv_bits}) b->new_call();
  SDF_HIP(ctx->cv_bits.reserve_exact(bits_bytes));
  SDF_HIP(ctx->cv_out.reserve(n_regions * sizeof(sdf_cover_counts)));
  if (int rc = upload_all(ctx, st, {{ctx->cv_regions, L.regions.data(), n_regions * sizeof(CoverRegion)},
                                    {ctx->cv_iv, L.iv.data(), n_iv * sizeof(CoverIv)}}))
    return rc;
  SDF_HIP(hipMemsetAsync(ctx->cv_bits.p, 0, bits_bytes, st));
  SDF_HIP(hipMemsetAsync(ctx->cv_out.p, 0, n_regions * sizeof(sdf_cover_counts), st));
  const char *pool = (const char *)ctx->an_pool.p;
  if (L.n_pieces) {
    SDF_HIP(ctx->cv_upper.reserve(n_iv * sizeof(int32_t)));
    SDF_HIP(hipMemsetAsync(ctx->cv_upper.p, 0, n_iv * sizeof(int32_t), st));
    const dim3 grid((unsigned)((L.n_pieces + 3) / 4));
    hipLaunchKernelGGL(cover_upper_kernel, grid, dim3(256), 0, st, (const CoverIv *)ctx->cv_iv.p, (int)n_iv, L.n_pieces, pool,
                       (int32_t *)ctx->cv_upper.p);
    hipLaunchKernelGGL(cover_paint_kernel, grid, dim3(256), 0, st, (const CoverIv *)ctx->cv_iv.p, (int)n_iv, L.n_pieces,
                       (const int32_t *)ctx->cv_upper.p, min_upper, L.set_words, (uint32_t *)ctx->cv_bits.p);
    ctx->launches += 2;
  }
  hipLaunchKernelGGL(cover_count_kernel, dim3((unsigned)((L.n_waves + 3) / 4)), dim3(256), 0, st, (const CoverRegion *)ctx->cv_regions.p,
                     (int)n_regions, L.n_waves, pool, (const uint32_t *)ctx->cv_bits.p, L.set_words, (sdf_cover_counts *)ctx->cv_out.p);
  ctx->launches += 1;
  SDF_HIP(hipGetLastError());
  SDF_HIP(hipMemcpyAsync(out, ctx->cv_out.p, n_regions * sizeof(sdf_cover_counts), hipMemcpyDeviceToHost, st));
  if (L.n_pieces) SDF_HIP(hipMemcpyAsync(upper.data(), ctx->cv_upper.p, n_iv * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return finish();
}

// The host form: the same rules a base at a time, the bitmaps as two arrays of bytes per region.
extern "C" int sdf_pool_coverage_host(const char *pool, size_t pool_bytes, const sdf_pool_range *regions, size_t n_regions,
                                      const sdf_cover_interval *iv, size_t n_iv, int32_t min_upper, sdf_cover_counts *out, int32_t *iv_upper,
                                      uint8_t *iv_painted) {
  if (pool_bytes && !pool) return SDF_ERR_INVALID;
  std::string why;
  if (int rc = check_cover(regions, n_regions, iv, n_iv, pool_bytes, out, &why)) return rc;
  std::vector<int32_t> upper(n_iv, 0);
  for (size_t i = 0; i < n_iv; i++) {
    const char *p = pool + regions[iv[i].region].off + iv[i].start;
    for (int32_t x = 0; x < iv[i].len; x++) upper[i] += cover_upper((unsigned char)p[x]);
  }
  std::vector<uint8_t> painted(n_iv, 0);
  cover_painted_all(iv, n_iv, upper.data(), min_upper, painted.data());
  std::vector<std::vector<uint8_t>> sets(2 * n_regions);  // [2 * region + set], made when first painted
  for (size_t i = 0; i < n_iv; i++) {
    if (!painted[i] || iv[i].len == 0) continue;
    std::vector<uint8_t> &S = sets[2 * (size_t)iv[i].region + (size_t)iv[i].set];
    if (S.empty()) S.assign((size_t)regions[iv[i].region].len, 0);
    std::fill(S.begin() + iv[i].start, S.begin() + iv[i].start + iv[i].len, (uint8_t)1);
  }
  for (size_t r = 0; r < n_regions; r++) {
    sdf_cover_counts c{0, 0, 0, 0, 0, 0, 0};
    const std::vector<uint8_t> &A = sets[2 * r], &B = sets[2 * r + 1];
    const char *p = pool + regions[r].off;
    for (int32_t x = 0; x < regions[r].len; x++) {
      const bool a = !A.empty() && A[(size_t)x], b = !B.empty() && B[(size_t)x], u = cover_upper_base((unsigned char)p[x]);
      c.a += a, c.b += b, c.both += a && b, c.a_only += a && !b, c.b_only += b && !a;
      c.a_only_upper += a && !b && u, c.b_only_upper += b && !a && u;
    }
    out[r] = c;
  }
  if (iv_upper && n_iv) memcpy(iv_upper, upper.data(), n_iv * sizeof(int32_t));
  if (iv_painted && n_iv) memcpy(iv_painted, painted.data(), n_iv);
  return SDF_OK;
}
